"""Python host mirror of the reference's lgrngn call surface, on top of the C ABI (include/lcx.h).

Same names, argument meaning and error behaviour as the reference's Python bindings
(bindings/python/lgrngn.hpp:40-140, bindings/python/lib.cpp:366-434) so that tests written
for the reference read the same here:

    opts_init = lgrngn.opts_init_t(); opts_init.dry_distros = {(kappa, rd_insol): fun}
    prtcls = lgrngn.factory(lgrngn.backend_t.HIP, opts_init)
    prtcls.init(th, rv, rhod, Cx=..., Cz=...)
    prtcls.step_sync(opts, th, rv, rhod); prtcls.step_async(opts)
    prtcls.diag_all(); prtcls.diag_sd_conc(); numpy.frombuffer(prtcls.outbuf())

Errors reported by the library are raised as RuntimeError with the library's message
(the reference throws std::runtime_error, translated by Boost.Python to RuntimeError).
"""
import ctypes as C
import enum
import numpy as np

from . import _lib

# ----------------------------------------------------------------------------- enums
class _bp_enum(enum.IntEnum):
    """str() of a Boost.Python enum value is its bare name (the reference's scripts write e.g. str(RH_formula) into CSV keys)"""
    def __str__(self):
        return self.name
    __format__ = enum.Enum.__format__


class backend_t(_bp_enum):          # lgrngn/backend.hpp:8 + the two new slots
    undefined = 0
    serial = 1
    OpenMP = 2
    CUDA = 3
    multi_CUDA = 4
    HIP = 5
    multi_HIP = 6


class kernel_t(_bp_enum):           # lgrngn/kernel.hpp:8
    undefined = 0
    geometric = 1
    golovin = 2
    hall = 3
    hall_davis_no_waals = 4
    long = 5                            # the Python module's spelling (ref: bindings/python/lib.cpp, kernel_t::Long in C++)
    Long = 5
    onishi_hall = 6
    onishi_hall_davis_no_waals = 7
    hall_pinsky_1000mb_grav = 8
    hall_pinsky_cumulonimbus = 9
    hall_pinsky_stratocumulus = 10
    vohl_davis_no_waals = 11


class vt_t(_bp_enum):               # lgrngn/terminal_velocity.hpp:8
    undefined = 0
    beard76 = 1
    beard77 = 2
    beard77fast = 3
    khvorostyanov_spherical = 4
    khvorostyanov_nonspherical = 5


class as_t(_bp_enum):               # lgrngn/advection_scheme.hpp:8
    undefined = 0
    implicit = 1
    euler = 2
    pred_corr = 3


class RH_formula_t(_bp_enum):       # lgrngn/RH_formula.hpp:8
    pv_cc = 0
    rv_cc = 1
    pv_tet = 2
    rv_tet = 3


class chem_species_t(_bp_enum):        # common/chem.hpp:8-22 (= enum lcx_chem_species, include/lcx_chem.h): the VALUES are the header's,
    HNO3 = 0                           # whatever order bindings/python/lib.cpp:257-265 lists the names in
    NH3 = 1
    CO2 = 2
    SO2 = 3
    H2O2 = 4
    O3 = 5
    S_VI = 6
    H = 7


chem_gas_n = 6                         # the first six species are the trace gases (ambient_chem) and their dissolved forms


class dbg(enum.IntFlag):
    """opts_init.dbg_flags: test / measurement switches (include/lcx.h, enum lcx_dbg; no reference counterpart)"""
    NO_COND_PRE = 1 << 0
    NO_WAVE_FLAGS = 1 << 1
    EAGER_COMPACT = 1 << 2
    SHUFFLE_PHILOX = 1 << 3
    NO_DEFERRED_SORT = 1 << 4
    COND_NO_FOLD = 1 << 5
    COND_SORTED_ORDER = 1 << 6
    NO_OVERLAP = 1 << 7
    MULTI_NO_PEER = 1 << 8
    MULTI_SERIALIZE = 1 << 9
    TAG = 1 << 10
    KPA_ARRAY = 1 << 11
    HOST_SYNC_LOOP = 1 << 12
    COND_LEAN_R3 = 1 << 13
    EXCH_SORT_NOW = 1 << 14
    COND_TOMS_TWO_PASS = 1 << 15
    FINISH_STAGED = 1 << 16
    NO_RANK_OVERLAP = 1 << 17
    RANK_BY_COUNTING = 1 << 18
    COND_FOLD = 1 << 19
    COND_NO_LIST = 1 << 20
    COND_WQ = 1 << 21
    COND_WQ_CAP128 = 1 << 22
    COND_WQ_PF = 1 << 23
    COND_WQ_PF2 = 1 << 24
    COND_BUDGET = 1 << 25
    COND_PROBE = 1 << 26
    COND_NO_FUSED_SUBSTEPS = 1 << 27
    VTERM_INVALID_OWN_PASS = 1 << 28
    RLX_GLOBAL_ATOMICS = 1 << 29
    NO_RANK_IN_COAL = 1 << 30
    NO_COAL_SKIP = 1 << 31


class dbg2(enum.IntFlag):
    """opts_init.dbg_flags2 (include/lcx.h, enum lcx_dbg2)"""
    COAL_SKIP_COUNT = 1 << 0
    NO_COAL_RANK_EXIT = 1 << 1
    COAL_RANK_EXIT_ALWAYS = 1 << 2
    NO_COAL_PREVOTE = 1 << 3
    NO_COAL_CELL_LIST = 1 << 4
    COAL_CELL_LIST_ALWAYS = 1 << 5
    COAL_CELL_LIST_SMALL = 1 << 6
    NO_COAL_CMAX_FLOOR = 1 << 7
    COAL_CMAX_FLOOR_HIGH = 1 << 8


class cond_kernel(enum.IntEnum):
    """enum lcx_cond_kernel (include/lcx.h): the kernel of an object's last condensation launch, particles_t.mode()"""
    none = 0
    strict = 1
    fast_per_droplet_setup = 2
    lean = 3
    lean_sorted = 4
    fold_toms748 = 5
    lean_toms748 = 6
    lean_toms748_sorted = 7
    toms748_two_pass = 8
    lean_r3 = 9
    fold_lean = 10
    lean_wq = 11
    per_particle = 12
    substeps = 13


class cond_finish(enum.IntEnum):
    """enum lcx_cond_finish (include/lcx.h): the form of an object's last per-cell finish, state_u64("raw_cond_finish")"""
    none = 0
    ordered = 1
    lanes8 = 2
    direct = 3
    wave = 4


class src_t(_bp_enum):              # lgrngn/ccn_source.hpp:8
    off = 0
    simple = 1
    matching = 2


# common::output_names (common/output.hpp:26-42)
output_names = ["HNO3", "NH3", "CO2", "SO2", "H2O2", "O3", "S_VI", "H", "liquid_volume", "dry_volume",
                "particle_number", "ice_mass", "liquid_number", "ice_number"]

# ----------------------------------------------------------------------------- C structs (include/lcx.h)
DISTRO_FN = C.CFUNCTYPE(C.c_double, C.c_double, C.c_void_p)


class _distro_c(C.Structure):
    _fields_ = [("kappa", C.c_double), ("rd_insol", C.c_double), ("fn", DISTRO_FN), ("user", C.c_void_p),
                ("n_modes", C.c_int), ("mean_rd", C.c_double * 4), ("sdev", C.c_double * 4), ("n_stp", C.c_double * 4)]


class _dry_size_c(C.Structure):
    _fields_ = [("kappa", C.c_double), ("rd_insol", C.c_double), ("radius", C.c_double), ("conc", C.c_double),
                ("sd_count", C.c_int)]


class _rlx_distro_c(C.Structure):
    _fields_ = [("distro", _distro_c), ("kappa_min", C.c_double), ("kappa_max", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double)]


class _opts_init_c(C.Structure):
    _fields_ = [
        ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
        ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double), ("dt", C.c_double),
        ("sstp_cond", C.c_int), ("sstp_coal", C.c_int), ("sstp_cond_act", C.c_int), ("sstp_chem", C.c_int),
        ("x0", C.c_double), ("y0", C.c_double), ("z0", C.c_double), ("x1", C.c_double), ("y1", C.c_double), ("z1", C.c_double),
        ("sd_conc", C.c_ulonglong),
        ("sd_conc_large_tail", C.c_int), ("aerosol_independent_of_rhod", C.c_int), ("variable_dt_switch", C.c_int),
        ("sd_const_multi", C.c_ulonglong), ("n_sd_max", C.c_ulonglong),
        ("kernel", C.c_int), ("terminal_velocity", C.c_int), ("adve_scheme", C.c_int), ("RH_formula", C.c_int),
        ("kernel_parameters", C.POINTER(C.c_double)), ("n_kernel_parameters", C.c_int),
        ("chem_switch", C.c_int), ("coal_switch", C.c_int), ("sedi_switch", C.c_int), ("subs_switch", C.c_int),
        ("rlx_switch", C.c_int), ("turb_adve_switch", C.c_int), ("turb_cond_switch", C.c_int), ("turb_coal_switch", C.c_int),
        ("ice_switch", C.c_int), ("exact_sstp_cond", C.c_int), ("sstp_cond_mix", C.c_int), ("adaptive_sstp_cond", C.c_int),
        ("time_dep_ice_nucl", C.c_int),
        ("RH_max", C.c_double),
        ("sstp_cond_adapt_drw2_eps", C.c_double), ("sstp_cond_adapt_drw2_max", C.c_double), ("rc2_T", C.c_double),
        ("rng_seed", C.c_int), ("rng_seed_init", C.c_int), ("rng_seed_init_switch", C.c_int),
        ("dev_count", C.c_int), ("dev_id", C.c_int),
        ("w_LS", C.POINTER(C.c_double)), ("n_w_LS", C.c_int),
        ("SGS_mix_len", C.POINTER(C.c_double)), ("n_SGS_mix_len", C.c_int),
        ("aerosol_conc_factor", C.POINTER(C.c_double)), ("n_aerosol_conc_factor", C.c_int),
        ("rd_min", C.c_double), ("rd_max", C.c_double),
        ("no_ccn_at_init", C.c_int), ("open_side_walls", C.c_int), ("periodic_topbot_walls", C.c_int),
        ("src_type", C.c_int),
        ("th_dry", C.c_int), ("const_p", C.c_int),
        ("diag_incloud_time", C.c_int),
        ("dry_distros", C.POINTER(_distro_c)), ("n_dry_distros", C.c_int),
        ("dry_sizes", C.POINTER(_dry_size_c)), ("n_dry_sizes", C.c_int),
        ("n_x_tot", C.c_int), ("n_x_bfr", C.c_int), ("bcond_lft", C.c_int), ("bcond_rgt", C.c_int),
        ("strict_fp", C.c_int), ("cond_solver", C.c_int), ("reorder_every", C.c_int), ("stream_ordered", C.c_int),
        ("dbg_flags", C.c_uint), ("dbg_cond_budget", C.c_int), ("dbg_pack_delay_us", C.c_int), ("dbg_flags2", C.c_uint),
        ("src_x0", C.c_double), ("src_y0", C.c_double), ("src_z0", C.c_double),
        ("src_x1", C.c_double), ("src_y1", C.c_double), ("src_z1", C.c_double),
        ("rlx_bins", C.c_int), ("supstp_rlx", C.c_int), ("rlx_sd_per_bin", C.c_double), ("rlx_timescale", C.c_double),
        ("rlx_dry_distros", C.POINTER(_rlx_distro_c)), ("n_rlx_dry_distros", C.c_int),
        ("chem_rho", C.c_double),
    ]


class _src_distro_c(C.Structure):
    _fields_ = [("distro", _distro_c), ("sd_conc", C.c_ulonglong), ("supstp", C.c_int)]


class _src_size_c(C.Structure):
    _fields_ = [("kappa", C.c_double), ("rd_insol", C.c_double), ("radius", C.c_double), ("conc_per_s", C.c_double),
                ("sd_count", C.c_int), ("supstp", C.c_int)]


class _opts_c(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("adve", "sedi", "subs", "cond", "coal", "src", "rlx", "rcyc", "turb_adve",
                                        "turb_cond", "turb_coal", "ice_nucl", "chem_dsl", "chem_dsc", "chem_rct")] + \
               [("RH_max", C.c_double), ("dt", C.c_double),
                ("src_dry_distros", C.POINTER(_src_distro_c)), ("n_src_dry_distros", C.c_int),
                ("src_dry_sizes", C.POINTER(_src_size_c)), ("n_src_dry_sizes", C.c_int)]


class _arrinfo_c(C.Structure):
    _fields_ = [("data", C.c_void_p), ("strides", C.POINTER(C.c_ssize_t)), ("on_device", C.c_int)]


# ---- many selections and moments in one pass (include/lcx_diag.h)
DIAG_MAX_CLAUSES = 4
_DIAG_SEL = {"all": 0, "dry": 1, "wet": 2, "kappa": 3, "water": 4}       # enum LCX_DIAG_SEL_*
_DIAG_MOM = {"dry": 1, "wet": 2, "kappa": 3}                             # enum LCX_DIAG_*_MOM (0: LCX_DIAG_SD_CONC)


class _diag_clause_c(C.Structure):
    _fields_ = [("sel", C.c_int), ("lo", C.c_double), ("hi", C.c_double)]


class _diag_req_c(C.Structure):
    _fields_ = [("n_clauses", C.c_int), ("clause", _diag_clause_c * DIAG_MAX_CLAUSES), ("count", C.c_int), ("k", C.c_int)]


def diag_batch_expressible(call):
    """whether diag_batch serves (clauses, count): a chain of all / rng dry, wet, kappa / water selections, the first without _cons and
    every further one with it, counted by sd_conc or a dry / wet / kappa moment"""
    sel, cnt = call
    if not 1 <= len(sel) <= DIAG_MAX_CLAUSES:
        return False
    for i, s in enumerate(sel):
        if s[0] == "all":
            cons = i > 0                                   # (diag_all has no _cons form: a later one would start the chain anew)
            ok = len(s) == 1 and i == 0
        elif s[0] == "rng":
            ok, cons = len(s) == 5 and s[1] in _DIAG_MOM, bool(s[4]) if len(s) == 5 else None
        elif s[0] == "water":
            ok, cons = len(s) == 2, bool(s[1]) if len(s) == 2 else None
        else:
            return False
        if not ok or cons != (i > 0):
            return False
    return (cnt[0] == "sd_conc" and len(cnt) == 1) or (cnt[0] == "mom" and len(cnt) == 3 and cnt[1] in _DIAG_MOM)


def diag_batch_requests(reqs):
    """[(clauses, count)] in the notation of the classic calls -- clauses: ("all",), ("rng", "dry" | "wet" | "kappa", lo, hi, cons),
    ("water", cons); count: ("sd_conc",), ("mom", "dry" | "wet" | "kappa", k) -- as an array of lcx_diag_req_t"""
    arr = (_diag_req_c * max(1, len(reqs)))()
    for r, call in enumerate(reqs):
        if not diag_batch_expressible(call):
            raise ValueError("libcloudph++: diag_batch cannot express request %d: %r" % (r, call))
        sel, cnt = call
        arr[r].n_clauses = len(sel)
        for i, s in enumerate(sel):
            c = arr[r].clause[i]
            c.sel = _DIAG_SEL[s[1]] if s[0] == "rng" else _DIAG_SEL[s[0]]
            if s[0] == "rng":
                c.lo, c.hi = float(s[2]), float(s[3])
        arr[r].count, arr[r].k = (0, 0) if cnt[0] == "sd_conc" else (_DIAG_MOM[cnt[1]], int(cnt[2]))
    return arr


def diag_batch_calls(arr, n):
    """the inverse of diag_batch_requests"""
    sel_name = {v: k for k, v in _DIAG_SEL.items()}
    mom_name = {v: k for k, v in _DIAG_MOM.items()}
    reqs = []
    for r in range(n):
        sel = []
        for i in range(arr[r].n_clauses):
            c, cons = arr[r].clause[i], i > 0
            nm = sel_name[c.sel]
            sel.append(("all",) if nm == "all" else ("water", cons) if nm == "water" else ("rng", nm, c.lo, c.hi, cons))
        reqs.append((sel, ("sd_conc",) if arr[r].count == 0 else ("mom", mom_name[arr[r].count], arr[r].k)))
    return reqs


def diag_batch_check(reqs, lib=None):
    """lcx_diag_batch_check on a translated list or on an (array of lcx_diag_req_t, n) pair; needs no GPU.  Raises the library's text."""
    lib = lib if lib is not None else _lib.load()
    arr, n = reqs if isinstance(reqs, tuple) else (diag_batch_requests(reqs), len(reqs))
    if lib.lcx_diag_batch_check(arr, C.c_int(n)) != 0:
        lib.lcx_last_error.restype = C.c_char_p
        raise RuntimeError(lib.lcx_last_error().decode())


# ---- per-cell rate tables: what the collision, condensation and move rates below share
def _rates_out(tag, out, n_rows, n_cell):
    """(address, row stride in doubles, on_device) of an output array of a rate table: (n_rows, n_cell) doubles with unit stride along
    cells -- a writeable numpy array, or a DeviceArray for memory of the object's device"""
    if len(out.shape) != 2 or out.shape[0] != n_rows or out.shape[1] != n_cell:
        raise ValueError("libcloudph++: %s: out must be 2-D, (%d, n_cell)" % (tag, n_rows))
    if isinstance(out, DeviceArray):
        ptr, strides = out.ptr, out.strides
    else:
        if out.dtype != np.float64:
            raise ValueError("libcloudph++: %s: out must hold float64" % tag)
        if any(st % out.itemsize for st in out.strides) or not out.flags.writeable:
            raise ValueError("libcloudph++: %s: unsupported strides" % tag)
        ptr, strides = out.ctypes.data, [st // out.itemsize for st in out.strides]
    if n_cell > 1 and strides[1] != 1:
        raise ValueError("libcloudph++: %s: out must have unit stride along cells" % tag)
    if strides[0] < n_cell:
        raise ValueError("libcloudph++: %s: out's row stride is below n_cell" % tag)
    return ptr, strides[0], isinstance(out, DeviceArray)


def _rates_thresholds(tag, r_thr, n_max, zero_ok):
    """the thresholds as an enable entry takes them, from a scalar or a sequence: 1 .. n_max finite, strictly increasing radii"""
    r = [float(x) for x in np.atleast_1d(np.asarray(r_thr, dtype=np.float64)).ravel()]
    if not 1 <= len(r) <= n_max:
        raise ValueError("libcloudph++: %s: n_thr = %d is outside 1 .. %d" % (tag, len(r), n_max))
    if not all((x >= 0 if zero_ok else x > 0) and np.isfinite(x) for x in r):
        raise ValueError("libcloudph++: %s: every threshold must be %s and finite" % (tag, "non-negative" if zero_ok else "positive"))
    if any(b <= a for a, b in zip(r, r[1:])):
        raise ValueError("libcloudph++: %s: the thresholds must be strictly increasing" % tag)
    return r


def _rate_index(tag, names, name, t=0, n_thr=1, total=None, noun="row", arg="row"):
    """the row of a name of `names` at threshold t (or of the trailing row `total`), or of a row number, among len(names) n_thr rows
    (and that one)"""
    n_rows = len(names) * n_thr + (total is not None)
    if isinstance(name, str):
        if name.lower() == total:
            return n_rows - 1
        if name.lower() not in names:
            raise ValueError("libcloudph++: %s: unknown %s %r (one of %s)" % (tag, noun, name, ", ".join(names + ((total,) if total else ()))))
        t = int(t)
        if not 0 <= t < n_thr:
            raise ValueError("libcloudph++: %s: t = %d is outside 0 .. %d" % (tag, t, n_thr - 1))
        return len(names) * t + names.index(name.lower())
    w = int(name)
    if not 0 <= w < n_rows:
        raise ValueError("libcloudph++: %s: %s = %d is outside 0 .. %d" % (tag, arg, w, n_rows - 1))
    return w


# ---- collision rates per cell (include/lcx_coal_rates.h)
COAL_RATES = ("acnv_m3", "acnv_nc", "acnv_nr", "accr_m3", "accr_nc", "self_cloud_n", "self_rain_n")     # enum LCX_CR_*, in its order


def coal_rate_index(name):
    """LCX_CR_* of an accumulator's name (one of COAL_RATES, any letter case) or of its number"""
    return _rate_index("coal_rates", COAL_RATES, name, noun="accumulator", arg="which")


def coal_rates_threshold(r_thr):
    """the threshold radius as lcx_coal_rates_enable takes it: a positive, finite number"""
    r = float(r_thr)
    if not (r > 0 and np.isfinite(r)):
        raise ValueError("libcloudph++: coal_rates: r_thr must be positive and finite")
    return r


def coal_rates_out(out, n_cell):
    """(address, row stride in doubles, on_device) of an output array of coal_rates: (len(COAL_RATES), n_cell), see _rates_out"""
    return _rates_out("coal_rates", out, len(COAL_RATES), n_cell)


# ---- condensation rates per cell (include/lcx_cond_rates.h)
COND_RATES = ("above_dm3", "up_n", "up_m3", "down_n", "down_m3")     # enum LCX_CDR_*, in its order: the rows of one threshold
COND_RATES_MAX_THR = 4                                               # LCX_CDR_MAX_THR
COND_RATES_TOTAL = "total_dm3"                                       # the last row, 5 K


def cond_rates_thresholds(r_thr):
    """the thresholds as lcx_cond_rates_enable takes them, from a scalar or a sequence: 1 .. 4 positive, finite, strictly increasing radii"""
    return _rates_thresholds("cond_rates", r_thr, COND_RATES_MAX_THR, False)


def cond_rate_index(name, t=0, n_thr=COND_RATES_MAX_THR):
    """the row of a name of COND_RATES at threshold t (or of "total_dm3"), or of a row number, among 5 n_thr + 1 rows"""
    return _rate_index("cond_rates", COND_RATES, name, t, n_thr, total=COND_RATES_TOTAL)


def cond_rates_out(out, n_thr, n_cell):
    """(address, row stride in doubles, on_device) of an output array of cond_rates: (5 n_thr + 1, n_cell), see _rates_out"""
    return _rates_out("cond_rates", out, len(COND_RATES) * n_thr + 1, n_cell)


# ---- move rates per cell (include/lcx_move_rates.h)
MOVE_RATES = ("in_n", "in_m3", "out_n", "out_m3", "down_n", "down_m3", "up_n", "up_m3", "precip_n", "precip_m3")   # enum LCX_MVR_*, in its order
MOVE_RATES_MAX_THR = 4                                               # LCX_MVR_MAX_THR


def move_rates_thresholds(r_thr):
    """the thresholds as lcx_move_rates_enable takes them, from a scalar or a sequence: 1 .. 4 finite, strictly increasing radii, the first
    may be 0 (every droplet)"""
    return _rates_thresholds("move_rates", r_thr, MOVE_RATES_MAX_THR, True)


def move_rate_index(name, t=0, n_thr=MOVE_RATES_MAX_THR):
    """the row of a name of MOVE_RATES at threshold t, or of a row number, among 10 n_thr rows"""
    return _rate_index("move_rates", MOVE_RATES, name, t, n_thr)


def move_rates_out(out, n_thr, n_cell):
    """(address, row stride in doubles, on_device) of an output array of move_rates: (10 n_thr, n_cell), see _rates_out"""
    return _rates_out("move_rates", out, len(MOVE_RATES) * n_thr, n_cell)


# ---- tracked super-droplets (include/lcx_track.h)
TRACK_FIELDS = ("n", "x", "y", "z", "rw2", "rd3", "kappa", "vt", "cell", "T", "RH", "rv")      # enum LCX_TRK_*, in its order
TRACK_MAX = 1 << 20                                                  # LCX_TRK_MAX


def track_clauses(clauses):
    """clauses in diag_batch's notation -- ("all",), ("rng", "dry" | "wet" | "kappa", lo, hi), ("water",); a trailing cons flag as there
    is accepted and not read: the clauses are ANDed -- as (array of lcx_diag_clause_t, n)"""
    clauses = list(clauses)
    if not 1 <= len(clauses) <= DIAG_MAX_CLAUSES:
        raise ValueError("libcloudph++: track: n_clauses = %d is outside 1 .. %d" % (len(clauses), DIAG_MAX_CLAUSES))
    arr = (_diag_clause_c * DIAG_MAX_CLAUSES)()
    for i, s in enumerate(clauses):
        s = tuple(s)
        if s and s[0] == "all" and len(s) == 1:
            arr[i].sel = _DIAG_SEL["all"]
        elif s and s[0] == "water" and len(s) in (1, 2):
            arr[i].sel = _DIAG_SEL["water"]
        elif s and s[0] == "rng" and len(s) in (4, 5) and s[1] in _DIAG_MOM:
            arr[i].sel, arr[i].lo, arr[i].hi = _DIAG_SEL[s[1]], float(s[2]), float(s[3])
        else:
            raise ValueError("libcloudph++: track: cannot express clause %d: %r" % (i, s))
    return arr, len(clauses)


def track_box(box):
    """None, or the six bounds (x0, x1, y0, y1, z0, z1) as lcx_track_select takes them"""
    if box is None:
        return None
    b = [float(v) for v in np.asarray(box, dtype=np.float64).ravel()]
    if len(b) != 6:
        raise ValueError("libcloudph++: track: box must hold six bounds (x0, x1, y0, y1, z0, z1), not %d" % len(b))
    if not all(np.isfinite(v) for v in b):
        raise ValueError("libcloudph++: track: box: every bound must be finite")
    if any(b[2 * d] > b[2 * d + 1] for d in range(3)):
        raise ValueError("libcloudph++: track: box: lo > hi")
    return (C.c_double * 6)(*b)


def track_check(clauses, box=None, max_count=1, lib=None):
    """lcx_track_check on clauses in diag_batch's notation and a box of six numbers; needs no GPU.  Raises the library's text."""
    lib = lib if lib is not None else _lib.load()
    arr, n = track_clauses(clauses)
    b = None if box is None else (C.c_double * 6)(*[float(v) for v in box])
    if lib.lcx_track_check(arr, C.c_int(n), b, C.c_size_t(max_count)) != 0:
        lib.lcx_last_error.restype = C.c_char_p
        raise RuntimeError(lib.lcx_last_error().decode())


# ---- the budget of tracked droplets (include/lcx_track_budget.h)
TRACK_BUDGET_FIELDS = ("cond_dr3", "coal_dr3", "coal_drd3", "chem_drd3", "coal_dn", "coal_gains", "coal_gives")      # enum LCX_TRB_*, in its order


def track_budget_check_out(out, n_samples, n_tracked):
    """refuses an `out` of track_budget that is no DeviceArray of (n_samples, 7, n_tracked) doubles with unit stride along the droplets"""
    nf = len(TRACK_BUDGET_FIELDS)
    if out is None:
        return
    if not isinstance(out, DeviceArray) or len(out.shape) != 3 or tuple(out.shape) != (n_samples, nf, n_tracked):
        raise ValueError("libcloudph++: track budget: out must be a DeviceArray of shape (n_samples, %d, n_tracked) = (%d, %d, %d)"
                         % (nf, n_samples, nf, n_tracked))
    if n_tracked > 1 and out.strides[2] != 1:
        raise ValueError("libcloudph++: track budget: out must have unit stride along the droplets")


# ---- the particle dump (include/lcx_dump.h)
DUMP_FIELDS = TRACK_FIELDS + ("slot", "track", "incloud_time", "chem_hno3", "chem_nh3", "chem_co2", "chem_so2", "chem_h2o2", "chem_o3",
                              "chem_s_vi", "chem_h")                 # enum LCX_DMP_*, in its order: the twelve of a track record as
DUMP_DEFAULT_FIELDS = ("n", "x", "y", "z", "rw2", "rd3", "kappa")   # TRACK_FIELDS spells them, the others in lower case
_DUMP_INDEX = {f.lower(): i for i, f in enumerate(DUMP_FIELDS)}


def dump_fields(fields):
    """names of DUMP_FIELDS (any letter case), each at most once, as (array of int, n, the names as DUMP_FIELDS spells them) for lcx_dump"""
    if isinstance(fields, str):
        fields = (fields,)
    low = [str(f).lower() for f in fields]
    if not 1 <= len(low) <= len(DUMP_FIELDS):
        raise ValueError("libcloudph++: dump: n_fields = %d is outside 1 .. %d" % (len(low), len(DUMP_FIELDS)))
    for nm in low:
        if nm not in _DUMP_INDEX:
            raise ValueError("libcloudph++: dump: unknown field %r (one of %s)" % (nm, ", ".join(DUMP_FIELDS)))
        if low.count(nm) > 1:
            raise ValueError("libcloudph++: dump: field %r is given twice" % nm)
    ids = [_DUMP_INDEX[nm] for nm in low]
    return (C.c_int * len(ids))(*ids), len(ids), [DUMP_FIELDS[i] for i in ids]


def dump_check_out(out, n_fields, max_count):
    """refuses an `out` of dump that is no DeviceArray of (n_fields, max_count) doubles with unit stride along the droplets"""
    if out is None:
        return
    if not isinstance(out, DeviceArray) or len(out.shape) != 2 or tuple(out.shape) != (n_fields, max_count):
        raise ValueError("libcloudph++: dump: out must be a DeviceArray of shape (n_fields, max_count) = (%d, %d)" % (n_fields, max_count))
    if max_count > 1 and out.strides[1] != 1:
        raise ValueError("libcloudph++: dump: out must have unit stride along the droplets")
    if n_fields > 1 and out.strides[0] < max_count:
        raise ValueError("libcloudph++: dump: out's row stride is below max_count")


def dump_check(clauses=(("all",),), box=None, fields=DUMP_DEFAULT_FIELDS, lib=None):
    """lcx_dump_check on clauses in diag_batch's notation, a box of six numbers and field names or numbers; needs no GPU.  Raises the
    library's text."""
    lib = lib if lib is not None else _lib.load()
    arr, n = track_clauses(clauses)
    b = None if box is None else (C.c_double * 6)(*[float(v) for v in box])
    ids = [_DUMP_INDEX[f.lower()] if isinstance(f, str) else int(f) for f in fields]
    fa = (C.c_int * max(len(ids), 1))(*ids)
    if lib.lcx_dump_check(arr, C.c_int(n), b, fa, C.c_int(len(ids))) != 0:
        lib.lcx_last_error.restype = C.c_char_p
        raise RuntimeError(lib.lcx_last_error().decode())


# ---- the collision log (include/lcx_coal_log.h)
COAL_LOG_FIELDS = ("launch", "cell", "slot_d", "slot_r", "col_no", "n_d", "n_r", "rw2_d", "rw2_r", "rw2_new", "rd3_d", "rd3_r",
                   "vt_d", "vt_r")                                   # enum LCX_CLG_*, in its order


def coal_log_args(capacity, r_min=0.):
    """(capacity, r_min) as lcx_coal_log_enable takes them: a positive integer and a non-negative, finite number"""
    if isinstance(capacity, (bool, float)) or int(capacity) != capacity:
        raise ValueError("libcloudph++: coal_log: capacity must be an integer")
    cap, r = int(capacity), float(r_min)
    if cap == 0:
        raise ValueError("libcloudph++: coal_log: capacity == 0")
    if not 0 < cap <= (2 ** 64 - 1) // (8 * len(COAL_LOG_FIELDS)):
        raise ValueError("libcloudph++: coal_log: capacity = %d is outside what a list of %d rows can hold" % (cap, len(COAL_LOG_FIELDS)))
    if not (r >= 0 and np.isfinite(r)):
        raise ValueError("libcloudph++: coal_log: r_min must be non-negative and finite")
    return cap, r


def coal_log_check_out(out):
    """refuses an `out` of coal_log that is no DeviceArray of (len(COAL_LOG_FIELDS), cap_events) doubles with unit stride along the
    events; returns (cap_events, row stride)"""
    nf = len(COAL_LOG_FIELDS)
    if not isinstance(out, DeviceArray) or len(out.shape) != 2 or out.shape[0] != nf or out.shape[1] < 1:
        raise ValueError("libcloudph++: coal_log: out must be a DeviceArray of shape (%d, cap_events)" % nf)
    if out.shape[1] > 1 and out.strides[1] != 1:
        raise ValueError("libcloudph++: coal_log: out must have unit stride along the events")
    if out.strides[0] < out.shape[1]:
        raise ValueError("libcloudph++: coal_log: out's row stride is below cap_events")
    return out.shape[1], out.strides[0]


def coal_log_check(capacity, r_min=0., lib=None):
    """lcx_coal_log_check on the numbers as given; needs no GPU.  Raises the library's text."""
    lib = lib if lib is not None else _lib.load()
    if lib.lcx_coal_log_check(C.c_size_t(capacity), C.c_double(r_min)) != 0:
        lib.lcx_last_error.restype = C.c_char_p
        raise RuntimeError(lib.lcx_last_error().decode())


# ----------------------------------------------------------------------------- user-facing option structs
class lognormal:
    """Built-in sum of lognormal modes n(ln rd) (common/lognormal.hpp:25-37); evaluated natively,
    no Python callback per super-droplet."""

    def __init__(self, mean_rd, sdev, n_stp):
        self.mean_rd = np.atleast_1d(np.asarray(mean_rd, dtype=float))
        self.sdev = np.atleast_1d(np.asarray(sdev, dtype=float))
        self.n_stp = np.atleast_1d(np.asarray(n_stp, dtype=float))
        assert len(self.mean_rd) == len(self.sdev) == len(self.n_stp) <= 4

    def __call__(self, lnrd):
        return float(np.sum(self.n_stp / np.sqrt(2 * np.pi) / np.log(self.sdev) *
                            np.exp(-(lnrd - np.log(self.mean_rd)) ** 2 / 2. / np.log(self.sdev) ** 2)))


class expvolume:
    """Built-in exponential-in-volume spectrum n(ln r) = 3 n_zero (r / r_zero)^3 exp(-(r / r_zero)^3) (Shima et al. 2009; the function
    the reference's Golovin test passes, tests/python/physics/coalescence_golovin.py:41-44); evaluated natively (lcx_distro_t.n_modes = -1)."""

    def __init__(self, r_zero, n_zero):
        self.r_zero, self.n_zero = float(r_zero), float(n_zero)

    def __call__(self, lnrd):
        q = np.exp(lnrd) ** 3 / self.r_zero ** 3
        return float(self.n_zero * 3. * q * np.exp(-q))


def _fill_distro(d, key, fun, keep):
    """one lcx_distro_t from a (kappa, rd_insol) key and a spectrum: built-in forms natively, anything else as a host callback"""
    d.kappa, d.rd_insol = float(key[0]), float(key[1])
    if isinstance(fun, lognormal):
        d.n_modes = len(fun.mean_rd)
        for m in range(len(fun.mean_rd)):
            d.mean_rd[m], d.sdev[m], d.n_stp[m] = fun.mean_rd[m], fun.sdev[m], fun.n_stp[m]
    elif isinstance(fun, expvolume):
        d.n_modes = -1
        d.mean_rd[0], d.n_stp[0] = fun.r_zero, fun.n_zero
    else:
        cb = DISTRO_FN(lambda lnrd, user, _f=fun: float(_f(lnrd)))
        keep.append(cb)
        d.fn = cb


class opts_init_t:
    """opts_init_t<real_t> with the reference's field names and defaults (opts_init.hpp:29-253)."""

    def __init__(self):
        self.dry_distros = {}
        self.dry_sizes = {}
        self.nx = self.ny = self.nz = 0
        self.dx = self.dy = self.dz = 1.
        self.dt = 0.
        self.sstp_cond = self.sstp_coal = self.sstp_cond_act = self.sstp_chem = 1
        self.x0 = self.y0 = self.z0 = 0.
        self.x1 = self.y1 = self.z1 = 1.
        self.sd_conc = 0
        self.sd_conc_large_tail = False
        self.aerosol_independent_of_rhod = False
        self.variable_dt_switch = False
        self.sd_const_multi = 0
        self.n_sd_max = 0
        self.kernel = kernel_t.undefined
        self.terminal_velocity = vt_t.undefined
        self.adve_scheme = as_t.implicit
        self.RH_formula = RH_formula_t.pv_cc
        self.kernel_parameters = np.zeros(0)
        self.chem_switch = False
        self.coal_switch = True
        self.sedi_switch = True
        self.subs_switch = False
        self.rlx_switch = False
        self.turb_adve_switch = self.turb_cond_switch = self.turb_coal_switch = False
        self.ice_switch = False
        self.exact_sstp_cond = False
        self.sstp_cond_mix = True
        self.adaptive_sstp_cond = False
        self.time_dep_ice_nucl = False
        self.RH_max = .95
        self.sstp_cond_adapt_drw2_eps, self.sstp_cond_adapt_drw2_max, self.rc2_T = 1e-4, 4., 10.
        self.rng_seed = 44
        self.rng_seed_init = 44
        self.rng_seed_init_switch = False
        self.dev_count = 0
        self.dev_id = -1
        self.w_LS = np.zeros(0)
        self.SGS_mix_len = np.zeros(0)
        self.aerosol_conc_factor = np.zeros(0)
        self.rd_min = self.rd_max = -1.
        self.no_ccn_at_init = False
        self.open_side_walls = False
        self.periodic_topbot_walls = False
        self.src_type = src_t.off
        self.th_dry = True
        self.const_p = False
        self.diag_incloud_time = False
        # box of the aerosol source (src_type simple / matching; the spectra are in opts_t)
        self.src_x0 = self.src_y0 = self.src_z0 = self.src_x1 = self.src_y1 = self.src_z1 = 0.
        # aerosol relaxation (rlx_switch, opts.rlx): {kappa: [spectrum at STP, [kappa_min, kappa_max], [z_min, z_max]]}
        self.rlx_dry_distros = {}
        self.rlx_bins, self.rlx_timescale, self.rlx_sd_per_bin, self.supstp_rlx = 0, 1., 0., 1
        # aqueous chemistry (chem_switch, sstp_chem): density of the dry aerosol, > 0 with chem_switch
        self.chem_rho = 0.
        # extensions (include/lcx.h)
        self.n_x_tot = 0
        self.n_x_bfr = 0
        self.bcond_lft = self.bcond_rgt = 0
        # the API default since round 5: fast arithmetic with the reference's TOMS748 iterates (held to the strict bars in every test);
        # strict_fp = True is the opt-in IEEE-order mode, cond_solver = 0 the lean bracketed secant of bench.py's headline
        self.strict_fp = False
        self.cond_solver = 1          # fast arithmetic only: 1 the reference's TOMS748 iterates, 0 lean bracketed secant (include/lcx.h)
        self.reorder_every = 0
        self.stream_ordered = False   # device arrays: step_sync returns once its work is queued on lcx_stream (include/lcx.h)
        # test / measurement switches (include/lcx.h, enum lcx_dbg): all off in production
        self.dbg_flags = 0
        self.dbg_cond_budget = 0
        self.dbg_pack_delay_us = 0
        self.dbg_flags2 = 0

    def _to_c(self, keep):
        c = _opts_init_c()
        special = {"kernel_parameters", "n_kernel_parameters", "w_LS", "n_w_LS", "SGS_mix_len", "n_SGS_mix_len", "aerosol_conc_factor",
                   "n_aerosol_conc_factor", "dry_distros", "n_dry_distros", "dry_sizes", "n_dry_sizes", "rlx_dry_distros", "n_rlx_dry_distros"}
        for name, ctype in _opts_init_c._fields_:
            if name in special:
                continue
            v = getattr(self, name)
            setattr(c, name, float(v) if ctype is C.c_double else int(v))
        for name in ("kernel_parameters", "w_LS", "SGS_mix_len", "aerosol_conc_factor"):
            arr = np.ascontiguousarray(np.asarray(getattr(self, name), dtype=np.float64).ravel())
            keep.append(arr)
            setattr(c, name, arr.ctypes.data_as(C.POINTER(C.c_double)))
            setattr(c, "n_" + name, arr.size)
        # std::map iteration order = sorted by (kappa, rd_insol) (distro_t.hpp:17-21)
        keys = sorted(self.dry_distros.keys())
        darr = (_distro_c * max(1, len(keys)))()
        for i, k in enumerate(keys):
            _fill_distro(darr[i], k, self.dry_distros[k], keep)
        keep.append(darr)
        c.dry_distros = C.cast(darr, C.POINTER(_distro_c))
        c.n_dry_distros = len(keys)
        # dry_sizes: {(kappa, rd_insol): {radius: [conc, count]}}
        flat = []
        for k in sorted(self.dry_sizes.keys()):
            for r in sorted(self.dry_sizes[k].keys()):
                conc, cnt = self.dry_sizes[k][r]
                flat.append((float(k[0]), float(k[1]), float(r), float(conc), int(cnt)))
        sarr = (_dry_size_c * max(1, len(flat)))()
        for i, t in enumerate(flat):
            sarr[i].kappa, sarr[i].rd_insol, sarr[i].radius, sarr[i].conc, sarr[i].sd_count = t
        keep.append(sarr)
        c.dry_sizes = C.cast(sarr, C.POINTER(_dry_size_c))
        c.n_dry_sizes = len(flat)
        # rlx_dry_distros: std::map order = sorted by kappa (null pointer, zero count when empty)
        kappas = sorted(self.rlx_dry_distros.keys())
        if kappas:
            rarr = (_rlx_distro_c * len(kappas))()
            for i, k in enumerate(kappas):
                fun, kappa_rng, z_rng = self.rlx_dry_distros[k]
                _fill_distro(rarr[i].distro, (k, 0.), fun, keep)
                rarr[i].kappa_min, rarr[i].kappa_max = float(kappa_rng[0]), float(kappa_rng[1])
                rarr[i].z_min, rarr[i].z_max = float(z_rng[0]), float(z_rng[1])
            keep.append(rarr)
            c.rlx_dry_distros = C.cast(rarr, C.POINTER(_rlx_distro_c))
            c.n_rlx_dry_distros = len(kappas)
        return c


def rlx_layout(opts_init, spectrum=0, lib=None):
    """Size bins of aerosol relaxation for entry `spectrum` (in kappa order) of opts_init.rlx_dry_distros as an object in double lays
    them out (lcx_rlx_layout, include/lcx_rlx.h; needs no GPU): (bin edges in rd3 [n_bins + 1], expected STP concentration per bin [n_bins])."""
    lib = lib if lib is not None else _lib.load()
    keep = []
    c = opts_init._to_c(keep)
    n = C.c_int()

    def chk(rc):
        if rc != 0:
            lib.lcx_last_error.restype = C.c_char_p
            raise RuntimeError(lib.lcx_last_error().decode())
    chk(lib.lcx_rlx_layout(C.byref(c), C.c_int(spectrum), None, None, C.byref(n)))
    edges, conc = np.zeros(n.value + 1), np.zeros(n.value)
    chk(lib.lcx_rlx_layout(C.byref(c), C.c_int(spectrum), edges.ctypes.data_as(C.POINTER(C.c_double)),
                           conc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
    return edges, conc


def snapshot_describe(buf, lib=None):
    """what a snapshot() holds, as text (lcx_snapshot_describe, include/lcx_state.h; needs no GPU): the format and library versions,
    the counts, one line per section.  Raises RuntimeError with the library's text for a blob that does not validate."""
    lib = lib if lib is not None else _lib.load()
    a = np.frombuffer(buf, dtype=np.uint8)
    out = C.create_string_buffer(1 << 16)
    if lib.lcx_snapshot_describe(C.c_void_p(a.ctypes.data if a.size else None), C.c_size_t(a.size), out, C.c_size_t(len(out))) != 0:
        lib.lcx_last_error.restype = C.c_char_p
        raise RuntimeError(lib.lcx_last_error().decode())
    return out.value.decode()


class opts_t:
    """opts_t<real_t> (opts.hpp:20-50)."""

    def __init__(self):
        self.adve = self.sedi = self.cond = self.coal = True
        self.subs = self.src = self.rlx = self.rcyc = False
        self.turb_adve = self.turb_cond = self.turb_coal = self.ice_nucl = False
        self.chem_dsl = self.chem_dsc = self.chem_rct = False
        self.RH_max = 44.
        self.dt = -1.
        self.chem = False    # accepted for source compatibility with the reference's tests (no-op)
        self.chem_gas = {}   # a holder only, as in the reference's binding (the gases are passed as ambient_chem= to init / step_sync)
        # aerosol source (opts_init.src_type): {(kappa, rd_insol): (spectrum per second, sd_conc, supstp)} and
        # {(kappa, rd_insol): {radius: [concentration per second, sd_count, supstp]}}
        self.src_dry_distros = {}
        self.src_dry_sizes = {}

    def _to_c(self):
        c = _opts_c()
        for name, ctype in _opts_c._fields_:
            if ctype is not C.c_double and ctype is not C.c_int or name.startswith("n_src_"):
                continue
            v = getattr(self, name)
            setattr(c, name, float(v) if ctype is C.c_double else int(bool(v)))
        if not self.src_dry_distros and not self.src_dry_sizes:
            return c                                   # (null pointers, zero counts)
        keep = []                                      # callbacks and arrays live as long as the struct the caller holds
        keys = sorted(self.src_dry_distros.keys())     # std::map order
        if keys:
            darr = (_src_distro_c * len(keys))()
            for i, k in enumerate(keys):
                fun, sd_conc, supstp = self.src_dry_distros[k]
                _fill_distro(darr[i].distro, k, fun, keep)
                darr[i].sd_conc, darr[i].supstp = int(sd_conc), int(supstp)
            keep.append(darr)
            c.src_dry_distros = C.cast(darr, C.POINTER(_src_distro_c))
            c.n_src_dry_distros = len(keys)
        flat = []
        for k in sorted(self.src_dry_sizes.keys()):
            for r in sorted(self.src_dry_sizes[k].keys()):
                conc, cnt, supstp = self.src_dry_sizes[k][r]
                flat.append((float(k[0]), float(k[1]), float(r), float(conc), int(cnt), int(supstp)))
        if flat:
            sarr = (_src_size_c * len(flat))()
            for i, t in enumerate(flat):
                sarr[i].kappa, sarr[i].rd_insol, sarr[i].radius, sarr[i].conc_per_s, sarr[i].sd_count, sarr[i].supstp = t
            keep.append(sarr)
            c.src_dry_sizes = C.cast(sarr, C.POINTER(_src_size_c))
            c.n_src_dry_sizes = len(flat)
        c._keep = keep
        return c


# ----------------------------------------------------------------------------- particles
class DeviceArray:
    """A device-resident n-d array handed to init/step_sync instead of a numpy array
    (extension: lcx_arrinfo_t.on_device).  `ptr` is a raw device address, strides in elements."""

    def __init__(self, ptr, shape, strides=None):
        self.ptr = int(ptr)
        self.shape = tuple(shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(self.shape):
                strides.insert(0, acc)
                acc *= s
        self.strides = tuple(strides)


class DeviceArrays:
    """The field of a multi-device object kept as one device array per slab (extension: lcx_arrinfo_t.on_device == 2):
    ptrs[i] = raw address of slab i's planes on slab i's device, shape = the shape of ONE slab's array (all alike)."""

    def __init__(self, ptrs, shape, strides=None):
        self.ptrs = [int(p) for p in ptrs]
        one = DeviceArray(0, shape, strides)
        self.shape, self.strides = one.shape, one.strides


class particles_t:
    """particles_t<real_t, HIP>; with multi=True particles_t<real_t, multi_HIP>: one object over opts_init.dev_count devices of
    this process (lcx_create_multi, include/lcx.h) -- same calls, global arrays."""

    def __init__(self, opts_init, real_t=np.float64, lib=None, prefix="lcx_", multi=False, _borrowed=None):
        self._lib = lib if lib is not None else _lib.load()
        self._px = prefix
        self._keep = []
        self.real_t = np.dtype(real_t)
        self.opts_init = opts_init
        self._arr_keep = []
        self._owner = None
        if _borrowed is not None:                  # a slab of a multi-device object: the parent owns the handle
            self._h, self._owner = _borrowed
            return
        c = opts_init._to_c(self._keep)
        self._h = C.c_void_p()
        self._chk(self._f("create_multi" if multi else "create")(C.byref(c), C.c_int(self.real_t.itemsize), C.byref(self._h)))

    # -- multi-device objects
    @property
    def dev_count(self):
        n = C.c_int()
        self._chk(self._f("multi_dev_count")(self._h, C.byref(n)))
        return n.value

    def slab(self, i):
        """particles_t view of slab i of a multi-device object (state getters, set_particles, random replay), owned by the parent"""
        h = C.c_void_p()
        self._chk(self._f("multi_slab")(self._h, C.c_int(i), C.byref(h)))
        return particles_t(self.opts_init, self.real_t, lib=self._lib, prefix=self._px, _borrowed=(h, self))

    # -- plumbing
    def _f(self, name):
        f = getattr(self._lib, self._px + name)
        return f

    def _chk(self, rc):
        if rc != 0:
            f = self._f("last_error")
            f.restype = C.c_char_p
            raise RuntimeError(f().decode())

    def __del__(self):
        try:
            if getattr(self, "_owner", None) is not None:
                return
            if getattr(self, "_h", None) and self._h.value:
                self._f("destroy")(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def _arr(self, a):
        if a is None:
            return None
        ai = _arrinfo_c()
        if isinstance(a, DeviceArrays):
            st = (C.c_ssize_t * max(1, len(a.strides)))(*a.strides) if a.strides else (C.c_ssize_t * 1)(1)
            tab = (C.c_void_p * len(a.ptrs))(*a.ptrs)
            ai.data, ai.strides, ai.on_device = C.cast(tab, C.c_void_p).value, C.cast(st, C.POINTER(C.c_ssize_t)), 2
            self._arr_keep.append((st, tab))
            return ai
        if isinstance(a, DeviceArray):
            st = (C.c_ssize_t * max(1, len(a.strides)))(*a.strides) if a.strides else (C.c_ssize_t * 1)(1)
            ai.data, ai.strides, ai.on_device = a.ptr, C.cast(st, C.POINTER(C.c_ssize_t)), 1
            self._arr_keep.append(st)
            return ai
        if a.dtype != self.real_t:
            raise RuntimeError("libcloudph++: array dtype does not match real_t")
        if a.ndim == 0 or a.size == 0:
            raise RuntimeError("libcloudph++: empty array")
        if any(s % a.itemsize for s in a.strides):
            raise RuntimeError("libcloudph++: unsupported strides")
        # the reference passes numpy strides in elements (bindings/python/lgrngn.hpp np2ai)
        st = (C.c_ssize_t * a.ndim)(*[s // a.itemsize for s in a.strides])
        ai.data, ai.strides, ai.on_device = a.ctypes.data, C.cast(st, C.POINTER(C.c_ssize_t)), 0
        self._arr_keep.append((a, st))
        return ai

    @staticmethod
    def _p(ai):
        return C.byref(ai) if ai is not None else None

    def _chem(self, ambient_chem):
        """ambient_chem = {chem_species_t: array} -> const lcx_arrinfo_t *[6] indexed by species (include/lcx_chem.h); a species that the
        dict lacks is a null entry, which the library answers as the reference answers a map of the wrong size"""
        tab = (C.POINTER(_arrinfo_c) * chem_gas_n)()
        for k, a in ambient_chem.items():
            if not 0 <= int(k) < chem_gas_n:
                raise RuntimeError("libcloudph++: ambient_chem holds the trace gases only (HNO3, NH3, CO2, SO2, H2O2, O3)")
            ai = self._arr(a)
            self._arr_keep.append(ai)
            tab[int(k)] = C.pointer(ai)
        return tab

    # -- API (particles.hpp:17-134)
    def init(self, th, rv, rhod, p=None, Cx=None, Cy=None, Cz=None, ambient_chem=None):
        self._arr_keep = []
        a = [self._arr(x) for x in (th, rv, rhod, p, Cx, Cy, Cz)]
        if ambient_chem:
            self._chk(self._f("init_chem")(self._h, *[self._p(x) for x in a], self._chem(ambient_chem)))
        else:
            self._chk(self._f("init")(self._h, *[self._p(x) for x in a]))

    def sync_in(self, th, rv, rhod=None, Cx=None, Cy=None, Cz=None, diss_rate=None, ambient_chem=None):
        self._arr_keep = []
        a = [self._arr(x) for x in (th, rv, rhod, Cx, Cy, Cz, diss_rate)]
        if ambient_chem:
            self._chk(self._f("sync_in_chem")(self._h, *[self._p(x) for x in a], self._chem(ambient_chem)))
        else:
            self._chk(self._f("sync_in")(self._h, *[self._p(x) for x in a]))

    def step_cond(self, opts, th, rv, ambient_chem=None):
        self._arr_keep = []
        a = [self._arr(x) for x in (th, rv)]
        oc = opts._to_c()
        if ambient_chem:
            self._chk(self._f("step_cond_chem")(self._h, C.byref(oc), *[self._p(x) for x in a], self._chem(ambient_chem)))
        else:
            self._chk(self._f("step_cond")(self._h, C.byref(oc), *[self._p(x) for x in a]))

    def step_sync(self, opts, th, rv, rhod=None, Cx=None, Cy=None, Cz=None, diss_rate=None, ambient_chem=None):
        self._arr_keep = []
        a = [self._arr(x) for x in (th, rv, rhod, Cx, Cy, Cz, diss_rate)]
        oc = opts._to_c()
        if ambient_chem:
            self._chk(self._f("step_sync_chem")(self._h, C.byref(oc), *[self._p(x) for x in a], self._chem(ambient_chem)))
        else:
            self._chk(self._f("step_sync")(self._h, C.byref(oc), *[self._p(x) for x in a]))

    def diag_chem(self, species):
        self._chk(self._f("diag_chem")(self._h, C.c_int(int(species))))

    def step_async(self, opts):
        oc = opts._to_c()
        self._chk(self._f("step_async")(self._h, C.byref(oc)))

    def _diag0(name):
        def f(self):
            self._chk(self._f(name)(self._h))
        f.__name__ = name
        return f

    def _diag2(name):
        def f(self, a, b):
            self._chk(self._f(name)(self._h, C.c_double(a), C.c_double(b)))
        f.__name__ = name
        return f

    def _diagk(name):
        def f(self, k):
            self._chk(self._f(name)(self._h, C.c_int(int(k))))
        f.__name__ = name
        return f

    diag_sd_conc = _diag0("diag_sd_conc")
    diag_pressure = _diag0("diag_pressure")
    diag_temperature = _diag0("diag_temperature")
    diag_RH = _diag0("diag_RH")
    diag_all = _diag0("diag_all")
    diag_vel_div = _diag0("diag_vel_div")
    diag_water = _diag0("diag_water")
    diag_precip_rate = _diag0("diag_precip_rate")
    diag_RH_ge_Sc = _diag0("diag_RH_ge_Sc")
    diag_rw_ge_rc = _diag0("diag_rw_ge_rc")

    def diag_wet_mass_dens(self, rad, sig0):
        self._chk(self._f("diag_wet_mass_dens")(self._h, C.c_double(rad), C.c_double(sig0)))
    diag_max_rw = _diag0("diag_max_rw")
    diag_dry_rng = _diag2("diag_dry_rng")
    diag_wet_rng = _diag2("diag_wet_rng")
    diag_kappa_rng = _diag2("diag_kappa_rng")
    diag_dry_rng_cons = _diag2("diag_dry_rng_cons")
    diag_wet_rng_cons = _diag2("diag_wet_rng_cons")
    diag_kappa_rng_cons = _diag2("diag_kappa_rng_cons")
    diag_dry_mom = _diagk("diag_dry_mom")
    diag_wet_mom = _diagk("diag_wet_mom")
    diag_kappa_mom = _diagk("diag_kappa_mom")
    diag_incloud_time_mom = _diagk("diag_incloud_time_mom")
    diag_up_mom = _diagk("diag_up_mom")
    diag_vp_mom = _diagk("diag_vp_mom")
    diag_wp_mom = _diagk("diag_wp_mom")
    diag_water_cons = _diag0("diag_water_cons")

    # -- many selections and moments in one pass (include/lcx_diag.h; no reference counterpart)
    def diag_batch_info(self):
        """(requests per pass, bytes that a diag_batch with host output allocates at most)"""
        rpp, nb = C.c_int(), C.c_size_t()
        self._chk(self._f("diag_batch_info")(self._h, C.byref(rpp), C.byref(nb)))
        return rpp.value, nb.value

    def diag_batch(self, reqs, out=None):
        """what the loop `selections; count; outbuf()` over reqs gives, bit for bit, from one pass over the super-droplets per
        diag_batch_info()[0] requests.  reqs: see diag_batch_requests.  Returns an (n_req, n_cell) array of real_t; with out= (a 2-D
        numpy array, or a DeviceArray for memory of the object's device; unit stride along cells, row stride >= n_cell) fills and
        returns that.  The classic selection and outbuf() are left as they were."""
        arr, n_req = diag_batch_requests(reqs), len(reqs)
        n_cell = self.n_cell
        if out is None:
            out = np.zeros((n_req, n_cell), dtype=self.real_t)
        if len(out.shape) != 2 or out.shape[0] < n_req or out.shape[1] != n_cell:
            raise RuntimeError("libcloudph++: diag_batch: out must be 2-D, (n_req, n_cell)")
        on_device = isinstance(out, DeviceArray)
        if on_device:
            ptr, strides = out.ptr, out.strides
        else:
            if out.dtype != self.real_t:
                raise RuntimeError("libcloudph++: array dtype does not match real_t")
            if any(s % out.itemsize for s in out.strides) or not out.flags.writeable:
                raise RuntimeError("libcloudph++: unsupported strides")
            ptr, strides = out.ctypes.data, [s // out.itemsize for s in out.strides]
        if n_cell > 1 and strides[1] != 1:
            raise RuntimeError("libcloudph++: diag_batch: out must have unit stride along cells")
        stride = strides[0] if out.shape[0] > 1 else n_cell                    # (a single row's stride says nothing)
        self._chk(self._f("diag_batch")(self._h, arr, C.c_int(n_req), C.c_void_p(ptr), C.c_size_t(max(stride, 0)), C.c_int(int(on_device))))
        return out

    # -- per-cell rate tables: what the three families below share
    def _rates_info(self, fam, n_max):
        """(enabled, the thresholds as a tuple, calls tallied since enable or the last reset) of the cond_rates or the move_rates"""
        en, k, r, n = C.c_int(), C.c_int(), (C.c_double * n_max)(), C.c_ulonglong()
        self._chk(self._f(fam + "_info")(self._h, C.byref(en), C.byref(k), r, C.byref(n)))
        return bool(en.value), tuple(r[t] for t in range(k.value)), n.value

    def _rates_read(self, fam, n_rows, reset, out):
        """the table of family fam, (n_rows, n_cell) float64, into out or into a new numpy array; returns what it filled"""
        n_cell = self.n_cell
        arr = np.zeros((n_rows, n_cell), dtype=np.float64) if out is None else out
        ptr, stride, on_device = _rates_out(fam, arr, n_rows, n_cell)
        self._chk(self._f(fam + "_read")(self._h, C.c_void_p(ptr), C.c_size_t(stride), C.c_int(int(on_device)), C.c_int(int(bool(reset)))))
        return arr

    # -- collision rates per cell (include/lcx_coal_rates.h; no reference counterpart)
    def coal_rates_enable(self, r_thr):
        """start (or restart from zero) the per-cell sums of what collisions move between cloud (r_wet < r_thr) and rain; before or
        after init()"""
        self._chk(self._f("coal_rates_enable")(self._h, C.c_double(coal_rates_threshold(r_thr))))

    def coal_rates_disable(self):
        self._chk(self._f("coal_rates_disable")(self._h))

    def coal_rates_info(self):
        """(enabled, r_thr, coalescence launches tallied since enable or the last reset)"""
        en, r, n = C.c_int(), C.c_double(), C.c_ulonglong()
        self._chk(self._f("coal_rates_info")(self._h, C.byref(en), C.byref(r), C.byref(n)))
        return bool(en.value), r.value, n.value

    def coal_rates(self, reset=False, out=None):
        """the seven accumulators: a dict name (COAL_RATES) -> ndarray(n_cell) of float64; with out= (a (7, n_cell) float64 numpy array or
        DeviceArray of the object's device) fills and returns that.  reset: zero them behind the read."""
        arr = self._rates_read("coal_rates", len(COAL_RATES), reset, out)
        return {nm: arr[w] for w, nm in enumerate(COAL_RATES)} if out is None else out

    def diag_coal_rate(self, name):
        """fills outbuf() with one accumulator (a name of COAL_RATES or its number), normalised as a diag_*_mom result"""
        self._chk(self._f("diag_coal_rate")(self._h, C.c_int(coal_rate_index(name))))

    # -- condensation rates per cell (include/lcx_cond_rates.h; no reference counterpart)
    def cond_rates_enable(self, r_thr):
        """start (or restart from zero) the per-cell tally of what step_cond's condensation does relative to the threshold radii r_thr (a
        scalar or up to four increasing values); before or after init()"""
        r = cond_rates_thresholds(r_thr)
        self._chk(self._f("cond_rates_enable")(self._h, (C.c_double * len(r))(*r), C.c_int(len(r))))

    def cond_rates_disable(self):
        self._chk(self._f("cond_rates_disable")(self._h))

    def cond_rates_info(self):
        """(enabled, the thresholds as a tuple, step_cond calls tallied since enable or the last reset)"""
        return self._rates_info("cond_rates", COND_RATES_MAX_THR)

    def cond_rates(self, reset=False, out=None):
        """the rows: a dict with "total_dm3" (n_cell,) and "above_dm3", "up_n", "up_m3", "down_n", "down_m3" (K, n_cell), float64; with out= (a
        (5 K + 1, n_cell) float64 numpy array or DeviceArray of the object's device) fills and returns that.  reset: zero them behind the read."""
        n_per, n_thr = len(COND_RATES), max(len(self.cond_rates_info()[1]), 1)
        arr = self._rates_read("cond_rates", n_per * n_thr + 1, reset, out)
        if out is not None:
            return out
        res = {nm: arr[w:n_per * n_thr:n_per] for w, nm in enumerate(COND_RATES)}
        res[COND_RATES_TOTAL] = arr[n_per * n_thr]
        return res

    def diag_cond_rate(self, name_or_row, t=0):
        """fills outbuf() with one row (a name of COND_RATES at threshold t, "total_dm3", or a row number), normalised as a diag_*_mom result"""
        n_thr = max(len(self.cond_rates_info()[1]), 1)
        self._chk(self._f("diag_cond_rate")(self._h, C.c_int(cond_rate_index(name_or_row, t, n_thr))))

    # -- move rates per cell (include/lcx_move_rates.h; no reference counterpart)
    def move_rates_enable(self, r_thr):
        """start (or restart from zero) the per-cell tally of what step_async's move carries in, out, up, down and onto the ground, relative
        to the threshold radii r_thr (a scalar or up to four increasing values, the first may be 0); before or after init()"""
        r = move_rates_thresholds(r_thr)
        self._chk(self._f("move_rates_enable")(self._h, (C.c_double * len(r))(*r), C.c_int(len(r))))

    def move_rates_disable(self):
        self._chk(self._f("move_rates_disable")(self._h))

    def move_rates_info(self):
        """(enabled, the thresholds as a tuple, moves tallied since enable or the last reset)"""
        return self._rates_info("move_rates", MOVE_RATES_MAX_THR)

    def move_rates(self, reset=False, out=None):
        """the rows: a dict name of MOVE_RATES -> (K, n_cell) float64; with out= (a (10 K, n_cell) float64 numpy array or DeviceArray of the
        object's device) fills and returns that.  reset: zero them behind the read."""
        n_per, n_thr = len(MOVE_RATES), max(len(self.move_rates_info()[1]), 1)
        arr = self._rates_read("move_rates", n_per * n_thr, reset, out)
        return {nm: arr[w::n_per] for w, nm in enumerate(MOVE_RATES)} if out is None else out

    def diag_move_rate(self, name_or_row, t=0):
        """fills outbuf() with one row (a name of MOVE_RATES at threshold t, or a row number), normalised as a diag_*_mom result"""
        n_thr = max(len(self.move_rates_info()[1]), 1)
        self._chk(self._f("diag_move_rate")(self._h, C.c_int(move_rate_index(name_or_row, t, n_thr))))

    # -- tracked super-droplets (include/lcx_track.h; no reference counterpart)
    def track_enable(self, max_tracked, capacity=64, every=0):
        """start (or start over) tracking: room for max_tracked droplets and `capacity` samples; every > 0: every every-th step_async ends in
        a sample.  Before or after init()."""
        max_tracked, capacity, every = int(max_tracked), int(capacity), int(every)
        if not 1 <= max_tracked <= TRACK_MAX:
            raise ValueError("libcloudph++: track: max_tracked = %d is outside 1 .. %d" % (max_tracked, TRACK_MAX))
        if capacity < 1:
            raise ValueError("libcloudph++: track: capacity must be at least 1")
        if every < 0:
            raise ValueError("libcloudph++: track: every = %d < 0" % every)
        self._chk(self._f("track_enable")(self._h, C.c_size_t(max_tracked), C.c_size_t(capacity), C.c_int(every)))

    def track_disable(self):
        self._chk(self._f("track_disable")(self._h))

    def track_select(self, clauses=(("all",),), box=None, max_count=None):
        """mark droplets that satisfy every clause (see track_clauses) and lie in box (x0, x1, y0, y1, z0, z1), at most max_count of them
        (None: all the room), spread evenly over the storage; returns how many were taken"""
        arr, n = track_clauses(clauses)
        b = track_box(box)
        if max_count is None:
            max_count = TRACK_MAX
        max_count = int(max_count)
        if max_count < 1:
            raise ValueError("libcloudph++: track: max_count must be at least 1")
        got = C.c_size_t()
        self._chk(self._f("track_select")(self._h, arr, C.c_int(n), b, C.c_size_t(max_count), C.byref(got)))
        return got.value

    def track_select_slots(self, slots):
        """mark the given storage slots (indices into the raw_ state) in their order; returns how many were taken"""
        sl = np.asarray(slots).ravel()
        if sl.size and (not np.issubdtype(sl.dtype, np.integer) or (sl < 0).any()):
            raise ValueError("libcloudph++: track: slots must be non-negative integers")
        sl = np.ascontiguousarray(sl, dtype=np.uint64)
        got = C.c_size_t()
        self._chk(self._f("track_select_slots")(self._h, sl.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.c_size_t(sl.size), C.byref(got)))
        return got.value

    def track_sample(self):
        self._chk(self._f("track_sample")(self._h))

    def track_info(self):
        """dict: enabled, max_tracked, n_tracked, capacity, n_samples, dropped, every, scans"""
        en, ev = C.c_int(), C.c_int()
        mx, nt, cp, ns = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        dr, sc = C.c_ulonglong(), C.c_ulonglong()
        self._chk(self._f("track_info")(self._h, C.byref(en), C.byref(mx), C.byref(nt), C.byref(cp), C.byref(ns), C.byref(dr), C.byref(ev), C.byref(sc)))
        return {"enabled": en.value, "max_tracked": mx.value, "n_tracked": nt.value, "capacity": cp.value, "n_samples": ns.value,
                "dropped": dr.value, "every": ev.value, "scans": sc.value}

    def track(self, reset=False, out=None):
        """the samples held: a dict with one (n_samples, n_tracked) float64 array per name of TRACK_FIELDS, plus "steps" (uint64) and "time".
        With out= (a DeviceArray of the object's device, (n_samples, 12, n_tracked) doubles with unit stride along the droplets) the
        records go there instead and the dict holds "steps" and "time" only.  reset: empty the buffer behind the read."""
        info = self.track_info()
        ns, nt, nf = info["n_samples"], info["n_tracked"], len(TRACK_FIELDS)
        steps, time = np.zeros(max(ns, 1), dtype=np.uint64), np.zeros(max(ns, 1), dtype=np.float64)
        if out is None:
            arr = np.zeros((max(ns, 1), nf, max(nt, 1)), dtype=np.float64)
            ptr, ss, fs, on_device = arr.ctypes.data, nf * max(nt, 1), max(nt, 1), False
        else:
            if not isinstance(out, DeviceArray) or len(out.shape) != 3 or tuple(out.shape) != (ns, nf, nt):
                raise ValueError("libcloudph++: track: out must be a DeviceArray of shape (n_samples, %d, n_tracked) = (%d, %d, %d)" % (nf, ns, nf, nt))
            if nt > 1 and out.strides[2] != 1:
                raise ValueError("libcloudph++: track: out must have unit stride along the droplets")
            ptr, ss, fs, on_device = out.ptr, out.strides[0], out.strides[1], True
        got = C.c_size_t()
        self._chk(self._f("track_read")(self._h, C.c_void_p(ptr), C.c_size_t(ss), C.c_size_t(fs), steps.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                        time.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(steps.size), C.byref(got), C.c_int(int(on_device)),
                                        C.c_int(int(bool(reset)))))
        res = {"steps": steps[:ns].copy(), "time": time[:ns].copy()}
        if out is None:
            for f, nm in enumerate(TRACK_FIELDS):
                res[nm] = arr[:ns, f, :nt].copy()
        return res

    # -- the budget of tracked droplets (include/lcx_track_budget.h)
    def track_budget_enable(self):
        """from now on every tracked droplet's growth is split by process (TRACK_BUDGET_FIELDS); needs track_enable"""
        self._chk(self._f("track_budget_enable")(self._h))

    def track_budget_disable(self):
        self._chk(self._f("track_budget_disable")(self._h))

    def track_budget_info(self):
        """dict: enabled, cond_passes, chem_passes, coal_passes"""
        en, cd, ch, co = C.c_int(), C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self._chk(self._f("track_budget_info")(self._h, C.byref(en), C.byref(cd), C.byref(ch), C.byref(co)))
        return {"enabled": en.value, "cond_passes": cd.value, "chem_passes": ch.value, "coal_passes": co.value}

    def track_budget(self, out=None):
        """the rows of the samples held: a dict with one (n_samples, n_tracked) float64 array per name of TRACK_BUDGET_FIELDS, plus "now":
        {name: (n_tracked,) array}, the accumulators as they stand.  With out= (a DeviceArray of the object's device, (n_samples, 7,
        n_tracked) doubles with unit stride along the droplets) the rows go there instead and the dict holds "now" only."""
        info = self.track_info()
        ns, nt, nf = info["n_samples"], info["n_tracked"], len(TRACK_BUDGET_FIELDS)
        track_budget_check_out(out, ns, nt)
        now = np.zeros((nf, max(nt, 1)), dtype=np.float64)
        nowp = now.ctypes.data_as(C.POINTER(C.c_double))
        got = C.c_size_t()
        call = self._f("track_budget_read")
        if out is None:
            arr = np.zeros((max(ns, 1), nf, max(nt, 1)), dtype=np.float64)
            self._chk(call(self._h, C.c_void_p(arr.ctypes.data), C.c_size_t(nf * max(nt, 1)), C.c_size_t(max(nt, 1)), C.c_size_t(max(ns, 1)), C.byref(got),
                           nowp, C.c_size_t(max(nt, 1)), C.c_int(0)))
        else:                                                                 # (the accumulators come to the host all the same: a call of their own)
            self._chk(call(self._h, C.c_void_p(out.ptr), C.c_size_t(out.strides[0]), C.c_size_t(out.strides[1]), C.c_size_t(ns), C.byref(got),
                           None, C.c_size_t(0), C.c_int(1)))
            self._chk(call(self._h, None, C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.byref(got), nowp, C.c_size_t(max(nt, 1)), C.c_int(0)))
        res = {"now": {nm: now[f, :nt].copy() for f, nm in enumerate(TRACK_BUDGET_FIELDS)}}
        if out is None:
            for f, nm in enumerate(TRACK_BUDGET_FIELDS):
                res[nm] = arr[:ns, f, :nt].copy()
        return res

    # -- the particle dump (include/lcx_dump.h; no reference counterpart)
    def _dump_call(self, arr, n, b, fa, nf, ptr, field_stride, max_count, on_device):
        q, w, st = C.c_size_t(), C.c_size_t(), C.c_ulonglong()
        self._chk(self._f("dump")(self._h, arr, C.c_int(n), b, fa, C.c_int(nf), C.c_void_p(ptr), C.c_size_t(field_stride), C.c_size_t(max_count),
                                  C.c_int(int(on_device)), C.byref(q), C.byref(w), C.byref(st)))
        return q.value, w.value, st.value

    def dump_count(self, clauses=(("all",),), box=None):
        """Q: how many droplets satisfy every clause (see track_clauses) and lie in box (x0, x1, y0, y1, z0, z1); nothing is written"""
        arr, n = track_clauses(clauses)
        fa = (C.c_int * 1)(0)
        return self._dump_call(arr, n, track_box(box), fa, 1, None, 0, 0, False)[0]

    def dump(self, clauses=(("all",),), box=None, fields=DUMP_DEFAULT_FIELDS, max_count=None, out=None):
        """the chosen fields (names of DUMP_FIELDS) of every qualifying droplet, in storage order: a dict {field: float64 array of n_written}
        plus "n_qualifying" and "stride" (ints).  max_count=None: count first, then everything; otherwise at most max_count droplets, every
        stride-th of the qualifying ones.  With out= (a DeviceArray of the object's device, (len(fields), max_count) doubles with unit
        stride along the droplets) the values go there, row f holding fields[f], and the dict holds the counts and "n_written" only.
        The object is only read: nothing is compacted, sorted or drawn."""
        arr, n = track_clauses(clauses)
        b = track_box(box)
        fa, nf, names = dump_fields(fields)
        if out is not None:
            if max_count is None:
                max_count = out.shape[1] if isinstance(out, DeviceArray) and len(out.shape) == 2 else 0
            max_count = int(max_count)
            if max_count < 1:
                raise ValueError("libcloudph++: dump: max_count must be at least 1")
            dump_check_out(out, nf, max_count)
            Q, w, st = self._dump_call(arr, n, b, fa, nf, out.ptr, out.strides[0] if nf > 1 else max(out.strides[0], max_count), max_count, True)
            return {"n_qualifying": Q, "stride": st, "n_written": w}
        if max_count is None:
            max_count = max(self._dump_call(arr, n, b, fa, nf, None, 0, 0, False)[0], 1)
        max_count = int(max_count)
        if max_count < 1:
            raise ValueError("libcloudph++: dump: max_count must be at least 1")
        host = np.zeros((nf, max_count), dtype=np.float64)
        Q, w, st = self._dump_call(arr, n, b, fa, nf, host.ctypes.data, max_count, max_count, False)
        res = {nm: host[f, :w].copy() for f, nm in enumerate(names)}
        res["n_qualifying"], res["stride"] = Q, st
        return res

    # -- the collision log (include/lcx_coal_log.h; no reference counterpart)
    def coal_log_enable(self, capacity, r_min=0.):
        """start (or restart, emptied) the list of coalescence events with room for `capacity` of them; r_min > 0 keeps only the events
        whose product has a wet radius of at least r_min.  Before or after init()"""
        cap, r = coal_log_args(capacity, r_min)
        self._chk(self._f("coal_log_enable")(self._h, C.c_size_t(cap), C.c_double(r)))

    def coal_log_disable(self):
        self._chk(self._f("coal_log_disable")(self._h))

    def coal_log_info(self):
        """(enabled, capacity, r_min, held, seen, launches): seen counts the logged events since enable or the last resetting read, held =
        min(seen, capacity) of them are in the list; launches counts coalescence launches since enable"""
        en, cap, r, held, seen, n = C.c_int(), C.c_size_t(), C.c_double(), C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self._chk(self._f("coal_log_info")(self._h, C.byref(en), C.byref(cap), C.byref(r), C.byref(held), C.byref(seen), C.byref(n)))
        return bool(en.value), cap.value, r.value, held.value, seen.value, n.value

    def coal_log(self, reset=False, out=None):
        """the held events: a dict name (COAL_LOG_FIELDS) -> float64 array of length held, in no particular order (coal_log_info has seen).  With
        out= (a DeviceArray of the object's device, (len(COAL_LOG_FIELDS), cap_events) doubles with unit stride along the events,
        cap_events >= held) the rows stay there, row f holding COAL_LOG_FIELDS[f], and the dict holds "n_written" and "seen" only.
        reset: empty the log behind the read."""
        nf = len(COAL_LOG_FIELDS)
        w, seen = C.c_size_t(), C.c_ulonglong()
        if out is not None:
            cap_events, stride = coal_log_check_out(out)
            self._chk(self._f("coal_log_read")(self._h, C.c_void_p(out.ptr), C.c_size_t(stride), C.c_size_t(cap_events), C.c_int(1),
                                               C.c_int(int(bool(reset))), C.byref(w), C.byref(seen)))
            return {"n_written": w.value, "seen": seen.value}
        info = self.coal_log_info()
        if not info[0]:
            raise RuntimeError("libcloudph++: coal_log: read while the log is not enabled (lcx_coal_log_enable)")
        room = max(info[3], 1)
        host = np.zeros((nf, room), dtype=np.float64)
        self._chk(self._f("coal_log_read")(self._h, C.c_void_p(host.ctypes.data), C.c_size_t(room), C.c_size_t(room), C.c_int(0),
                                           C.c_int(int(bool(reset))), C.byref(w), C.byref(seen)))
        return {nm: host[f, :w.value].copy() for f, nm in enumerate(COAL_LOG_FIELDS)}

    def outbuf(self):
        """bytes-like view of n_cell reals (use numpy.frombuffer(..., dtype=real_t), default float64)."""
        ptr, n = C.c_void_p(), C.c_size_t()
        self._chk(self._f("outbuf")(self._h, C.byref(ptr), C.byref(n)))
        buf = (C.c_char * (n.value * self.real_t.itemsize)).from_address(ptr.value)
        return memoryview(buf)

    def outbuf_array(self):
        return np.frombuffer(self.outbuf(), dtype=self.real_t).copy()

    def get_attr(self, name):
        n = C.c_size_t()
        self._chk(self._f("get_attr")(self._h, name.encode(), None, C.c_size_t(0), C.byref(n)))
        out = np.empty(n.value, dtype=self.real_t)
        self._chk(self._f("get_attr")(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(n)))
        return out

    def diag_puddle(self):
        out = (C.c_double * len(output_names))()
        self._chk(self._f("diag_puddle")(self._h, out))
        return {nm: out[i] for i, nm in enumerate(output_names)}

    # -- introspection hooks (no reference counterpart)
    @property
    def n_part(self):
        n = C.c_size_t()
        self._chk(self._f("n_part")(self._h, C.byref(n)))
        return n.value

    @property
    def n_cell(self):
        n = C.c_size_t()
        self._chk(self._f("n_cell")(self._h, C.byref(n)))
        return n.value

    def state_u64(self, name):
        n = C.c_size_t()
        self._chk(self._f("get_state_u64")(self._h, name.encode(), None, C.c_size_t(0), C.byref(n)))
        out = np.empty(n.value, dtype=np.uint64)
        self._chk(self._f("get_state_u64")(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                           C.c_size_t(out.size), C.byref(n)))
        return out

    def state_real(self, name):
        n = C.c_size_t()
        self._chk(self._f("get_state_real")(self._h, name.encode(), None, C.c_size_t(0), C.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        self._chk(self._f("get_state_real")(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)),
                                            C.c_size_t(out.size), C.byref(n)))
        return out

    def set_particles(self, n, rd3, rw2, kpa, vt, x=None, y=None, z=None):
        def d(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            self._arr_keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_double))
        nn = np.ascontiguousarray(n, dtype=np.uint64)
        self._chk(self._f("set_particles")(self._h, C.c_size_t(nn.size), nn.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                           d(rd3), d(rw2), d(kpa), d(vt), d(x), d(y), d(z)))

    def rng_replay_push(self, kind, data):
        a = np.ascontiguousarray(data, dtype=np.float64)
        self._chk(self._f("rng_replay_push")(self._h, C.c_int(kind), a.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(a.size)))

    def set_state_real(self, name, data):
        """test hook of tests/test_hip_reverse_replay.py (the product sets "tag" only; the oracle also rw2, th, rv)"""
        a = np.ascontiguousarray(data, dtype=np.float64)
        self._chk(self._f("set_state_real")(self._h, name.encode(), a.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(a.size)))

    def rng_replay_pending(self):
        n = C.c_size_t()
        self._chk(self._f("rng_replay_pending")(self._h, C.byref(n)))
        return n.value

    def rng_dump(self, call, which):
        """what coalescence call `call` of the last step_async consumed of the generator (lcx_rng_dump; needs dbg.TAG)"""
        n = C.c_size_t()
        self._chk(self._f("rng_dump")(self._h, C.c_int(call), C.c_int(which), None, C.c_size_t(0), C.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        self._chk(self._f("rng_dump")(self._h, C.c_int(call), C.c_int(which), out.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.c_size_t(out.size), C.byref(n)))
        return out

    def stage(self, name, opts=None):
        oc = opts._to_c() if opts is not None else None
        self._chk(self._f("stage")(self._h, name.encode(), C.byref(oc) if oc is not None else None))

    def timings(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        n = C.c_size_t()
        self._chk(self._f("timings")(self._h, names, ms, C.c_size_t(cap), C.byref(n)))
        return {names[i].decode(): ms[i] for i in range(n.value)}

    def mode(self):
        """what the OBJECT runs (lcx_get_state_u64 "raw_mode"): (strict_fp, cond_solver, cond_kernel of the last condensation launch,
        dbg_flags) -- a test that claims the benchmarked or the default path asserts these instead of trusting what it meant to set"""
        v = self.state_u64("raw_mode")
        return bool(v[0]), int(v[1]), cond_kernel(int(v[2])), dbg(int(v[3]))

    def move_kernel(self):
        """the k_move instantiation of the object's last move launch (lcx_get_state_u64 "raw_move_kernel"): (PC, TURB, SPEC), SPEC the
        sum of 1 three-dimensional, 2 the full step's pass, 4 a slab with neighbours, 8 implicit"""
        v = int(self.state_u64("raw_move_kernel")[0])
        return bool(v & 16), bool(v & 32), v & 15

    def set_profiling(self, on):
        self._chk(self._f("set_profiling")(self._h, C.c_int(int(on))))

    # -- 1-D decomposition primitives
    def migrate_counts(self):
        l, r = C.c_size_t(), C.c_size_t()
        self._chk(self._f("migrate_counts")(self._h, C.byref(l), C.byref(r)))
        return l.value, r.value

    def courant_halo_count(self, which):
        f = self._f("courant_halo_count")
        f.restype = C.c_size_t
        return int(f(self._h, C.c_int(which)))

    def courant_halo_pack(self, which, side, ptr):
        self._chk(self._f("courant_halo_pack")(self._h, C.c_int(which), C.c_int(side), C.c_void_p(ptr)))

    def courant_halo_unpack(self, which, side, ptr):
        self._chk(self._f("courant_halo_unpack")(self._h, C.c_int(which), C.c_int(side), C.c_void_p(ptr)))

    def migrate_record_bytes(self):
        f = self._f("migrate_record_bytes")
        f.restype = C.c_size_t
        return f(self._h)

    def migrate_pack(self, side, x_rmt, buf_ptr, cap_bytes):
        self._chk(self._f("migrate_pack")(self._h, C.c_int(side), C.c_double(x_rmt), C.c_void_p(buf_ptr), C.c_size_t(cap_bytes)))

    def migrate_unpack(self, buf_ptr, count):
        self._chk(self._f("migrate_unpack")(self._h, C.c_void_p(buf_ptr), C.c_size_t(count)))

    def migrate_finish(self, opts):
        oc = opts._to_c()
        self._chk(self._f("migrate_finish")(self._h, C.byref(oc)))

    # -- the device-driven exchange for one process per GPU (include/lcx.h lcx_exch_*; driven by libcloudphxx_amd.multi)
    def exch_enable(self, nx_min):
        cap = C.c_size_t()
        self._chk(self._f("exch_enable")(self._h, C.c_int(nx_min), C.byref(cap)))
        return cap.value

    def exch_buffers(self):
        """addresses of (outbox to the left, outbox to the right, inbox from the left, inbox from the right)"""
        p4 = (C.c_void_p * 4)()
        self._chk(self._f("exch_buffers")(self._h, p4))
        return [int(v or 0) for v in p4]

    def exch_message_bytes(self, n_rec):
        f = self._f("exch_message_bytes")
        f.restype = C.c_size_t
        return f(self._h, C.c_size_t(n_rec))

    def exch_pack(self, has_lft, lft_x1, has_rgt, rgt_x0, next_cap_lft=0, next_cap_rgt=0):
        self._chk(self._f("exch_pack")(self._h, C.c_int(bool(has_lft)), C.c_double(lft_x1), C.c_int(bool(has_rgt)), C.c_double(rgt_x0),
                                       C.c_uint(next_cap_lft), C.c_uint(next_cap_rgt)))

    def exch_sort_interior(self):
        self._chk(self._f("exch_sort_interior")(self._h))

    def exch_unpack(self, from_lft, from_rgt, have_lft=0xFFFFFFFF, have_rgt=0xFFFFFFFF):
        self._chk(self._f("exch_unpack")(self._h, C.c_int(bool(from_lft)), C.c_int(bool(from_rgt)), C.c_uint(have_lft), C.c_uint(have_rgt)))

    def exch_finish(self, opts):
        """the step's one host synchronisation: (complete, record) -- record = [dead, out_lft, out_rgt, in_lft, in_rgt, flags, crowded
        cells, largest cell, shift, next_cap_lft, next_cap_rgt, 0]"""
        oc = opts._to_c()
        rec = (C.c_uint * 12)()
        done = C.c_int()
        self._chk(self._f("exch_finish")(self._h, C.byref(oc), rec, C.byref(done)))
        return bool(done.value), list(rec)

    # -- checkpoint and restart (include/lcx_state.h)
    def snapshot(self):
        """everything this object needs in order to go on, as one numpy array of uint8 (lcx_snapshot_save); taken after init() or after
        step_async().  Taking it cannot be observed in this object's results."""
        n = C.c_size_t()
        self._chk(self._f("snapshot_size")(self._h, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        self._chk(self._f("snapshot_save")(self._h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value]

    def restore(self, buf):
        """in the place of init(), on a fresh object made from the same opts_init and real_t: load a snapshot() (any object with the
        buffer protocol) and be where the saved object was -- the next call is step_sync.  The caller keeps his own fields and step counter."""
        a = np.frombuffer(buf, dtype=np.uint8)
        if not a.flags["C_CONTIGUOUS"]:
            a = np.ascontiguousarray(a)
        self._chk(self._f("snapshot_load")(self._h, C.c_void_p(a.ctypes.data if a.size else None), C.c_size_t(a.size)))

    def stream(self):
        """the hipStream_t (as an integer) every launch of this object is queued on; 0 for an engine without one"""
        p = C.c_void_p()
        self._chk(self._f("stream")(self._h, C.byref(p)))
        return int(p.value or 0)


def factory(backend, opts_init, real_t=np.float64):
    """factory<real_t>(backend, opts_init)  (factory.hpp:12-15, src/lib.cpp:13-40).

    Only the HIP backends exist in this library; asking for a backend that was not compiled in
    raises, as the reference does (src/lib.cpp:21,27,33,38)."""
    backend = backend_t(backend)
    if backend == backend_t.HIP or backend == backend_t.CUDA:
        return particles_t(opts_init, real_t)
    if backend in (backend_t.multi_HIP, backend_t.multi_CUDA):
        # one object, opts_init.dev_count devices of this process (0: all visible) -- the reference's multi_CUDA.  The SPMD flavour
        # (one process per GPU, torch.distributed) is libcloudphxx_amd.multi.particles_multi_t.
        return particles_t(opts_init, real_t, multi=True)
    raise RuntimeError("libcloudph++: backend %s not compiled in this library (available: HIP, multi_HIP)" % backend.name)
