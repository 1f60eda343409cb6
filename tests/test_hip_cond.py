"""Condensation of the HIP object, one object per condensation kernel (lgrngn.cond_kernel, read back from the object), double and
float, against tests/_cond_reference.py (numpy long double, written from the reference's sources, no project code) on the crafted
cases of tests/test_oracle_cond.py: subsaturated and supersaturated air, the bracket clamped to the dry radius, explicit Euler,
droplets on their dry radius, a negative Reynolds number, very uneven cells for the four per-cell finish kernels, the scalar-kappa
instantiations on an object straight from init, and the fused substeps.  The cases, the checks and the bars (measured on the CPU oracle,
never here) are in that module; WORST collects what the device reaches, for the record.

Two gaps, on purpose.  The object reports its condensation kernel and nothing about the per-cell finish: which of k_cond_cellfinish<T, 1>,
<T, 8>, _direct and _wave ran is what launch_cellfinish (lcx_core.hip) decides from the arithmetic, the order, FINISH_STAGED, the number
of cells and the mean occupancy -- the cases are laid out for those conditions as they stand (C asserts the two numbers it restates), and
a change of that dispatch would move them to another finish kernel without a test noticing.  And float runs strict, lean, fold_toms748
and lean_wq only: lean_r3, fold_lean, lean_sorted and the resume pass meet the reference in double alone."""
import numpy as np
import pytest

import _harness as h
import test_oracle_cond as O
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

D = lgrngn.dbg
WORST = {}

# name -> (strict_fp, cond_solver, dbg_flags, dbg_cond_budget, the kernel the object must report)
KERNELS = {
    "strict": (True, 0, 0, 0, "strict"),
    "fast_per_droplet_setup": (False, 0, D.NO_COND_PRE, 0, "fast_per_droplet_setup"),
    "lean": (False, 0, 0, 0, "lean"),
    "lean_sorted": (False, 0, D.COND_SORTED_ORDER, 0, "lean_sorted"),
    "fold_toms748": (False, 1, 0, 0, "fold_toms748"),
    "lean_toms748": (False, 1, D.COND_NO_FOLD, 0, "lean_toms748"),
    "lean_toms748_sorted": (False, 1, D.COND_SORTED_ORDER, 0, "lean_toms748_sorted"),
    "toms748_two_pass_3": (False, 1, D.COND_TOMS_TWO_PASS, 3, "toms748_two_pass"),
    "toms748_two_pass_all": (False, 1, D.COND_TOMS_TWO_PASS, -1, "toms748_two_pass"),
    "lean_r3": (False, 0, D.COND_LEAN_R3, 0, "lean_r3"),
    "fold_lean": (False, 0, D.COND_FOLD, 0, "fold_lean"),
    "lean_wq": (False, 0, D.COND_WQ, 0, "lean_wq"),
    "lean_wq_cap128": (False, 0, D.COND_WQ | D.COND_WQ_CAP128, 0, "lean_wq"),
    "lean_resume_1": (False, 0, D.COND_BUDGET, 1, "lean"),
    "lean_resume_2": (False, 0, D.COND_BUDGET, 2, "lean"),
    "lean_finish_staged": (False, 0, D.FINISH_STAGED, 0, "lean"),
    "lean_sorted_finish_staged": (False, 0, D.COND_SORTED_ORDER | D.FINISH_STAGED, 0, "lean_sorted"),
}


def run(name, real_t, strict, solver, flags, budget, kernel, sstp=1, raw=False, case=None, sample=None):
    def make(oi, t):
        oi.strict_fp, oi.cond_solver, oi.dbg_flags, oi.dbg_cond_budget = strict, solver, int(flags), budget
        return h.hip_particles(oi, t)
    worst = WORST.setdefault(real_t.__name__, {})
    seen = O.run_case(name, make, real_t, sstp, worst=worst, fixed_point=not strict, raw=raw, case=case, sample=sample,
                      after_step=lambda prt: h.assert_mode(prt, strict, solver, kernel=kernel))
    print("\nhip cond %s %s sstp %d: worst so far %s branches %s" % (name, real_t.__name__, sstp, {k: round(v, 3) for k, v in worst.items()}, seen))


@pytest.mark.parametrize("which", list(KERNELS))
@pytest.mark.parametrize("name", ["W", "W_clamp", "U1", "U2"])
def test_every_condensation_kernel_f64(name, which):
    run(name, np.float64, *KERNELS[which])


@pytest.mark.parametrize("which", ["strict", "lean", "fold_toms748", "lean_wq"])
@pytest.mark.parametrize("name", ["W", "W_clamp", "U1", "U2"])
def test_condensation_kernels_f32(name, which):
    run(name, np.float32, *KERNELS[which])


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_substep"])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("name", ["W", "U1", "U2"])
def test_substeps(name, solver, fused, real_t):
    kernel = "substeps" if fused else ("lean", "fold_toms748")[solver]
    run(name, real_t, False, solver, 0 if fused else D.COND_NO_FUSED_SUBSTEPS, 0, kernel, sstp=4)


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("sstp", [1, 3])
@pytest.mark.parametrize("mode", ["api_default", "bench"])
def test_scalar_kappa_whole_steps(mode, sstp, real_t):
    """straight from init, nothing read but the raw storage: the UNI = true instantiations and the carried scatter of the production
    order"""
    h.api_default_opts(lgrngn.opts_init_t())
    strict, solver = (h.API_DEFAULTS["strict_fp"], h.API_DEFAULTS["cond_solver"]) if mode == "api_default" else (False, 0)
    assert not strict
    kernel = "substeps" if sstp > 1 else ("lean", "fold_toms748")[solver]
    run("S", real_t, strict, solver, 0, 0, kernel, sstp=sstp, raw=True)


def test_crowded_finish():
    """C: 16^3 cells at a mean above 192, k_cond_cellfinish_wave's territory (lcx_core.hip launch_cellfinish: fast arithmetic, at least
    4096 cells, at least 192 droplets per cell); cells of 0 .. 600 and one of 2100; every cell's closure, droplets on a fixed sample"""
    real_t = np.float64
    rng = np.random.default_rng(77)
    counts = rng.integers(0, 411, 4096)
    counts[::97] = 600
    counts[5::101] = 0
    counts[2000] = 2100
    oi = h.box_opts(16, 16, 16, 8, n_sd_max=int(counts.sum()) + 64)
    case = O.Case(oi, real_t, (.95, 1.02), 31, counts, heavy_cell=2000, branches=("implicit_up", "implicit_down"))
    assert counts.size >= 4096 and counts.sum() // counts.size >= 192
    run("C", real_t, False, 0, 0, 0, "lean", case=case, sample=rng.choice(int(counts.sum()), 20000, replace=False))
