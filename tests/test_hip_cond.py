"""Condensation of the HIP object, one object per condensation kernel (lgrngn.cond_kernel, read back from the object), double and
float, against tests/_cond_reference.py (numpy long double, written from the reference's sources, no project code) on the crafted
cases of tests/test_oracle_cond.py: subsaturated and supersaturated air, the bracket clamped to the dry radius, explicit Euler,
droplets on their dry radius, a negative Reynolds number, very uneven cells for the four per-cell finish kernels, the scalar-kappa
instantiations on an object straight from init, and the fused substeps.  The cases, the checks and the bars (measured on the CPU oracle,
never here) are in that module; WORST collects what the device reaches, for the record.

The object reports its condensation kernel and the form of its per-cell finish (lgrngn.cond_finish: k_cond_cellfinish<T, 1>, <T, 8>,
_direct, _wave, or none where k_cond_substeps finishes its cells itself), and every case asserts both after every step.

One gap, on purpose: float runs strict, lean, fold_toms748 and lean_wq only: lean_r3, fold_lean, lean_sorted and the resume pass meet
the reference in double alone."""
import numpy as np
import pytest

import _harness as h
import test_oracle_cond as O
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

D = lgrngn.dbg
WORST = {}

# name -> (strict_fp, cond_solver, dbg_flags, dbg_cond_budget, the kernel the object must report, the form of its per-cell finish)
# The finish, from the rules of launch_cellfinish as they stood before the object reported it, for a few hundred cells (never the 4096 of
# the wave's form): strict arithmetic walks each cell in order; fast arithmetic takes eight lanes per cell through the LDS stage where
# it has n rw^3 before and after (the per-droplet set-up), where the changes lie in storage order and must be gathered (a storage-order
# kernel that carried no scatter: these objects come straight from init, nothing deferred a sort) or where FINISH_STAGED asks for it; and
# reads the changes straight from the sorted order otherwise (the sorted-order kernels, and the two-pass form, which walks it too).
KERNELS = {
    "strict": (True, 0, 0, 0, "strict", "ordered"),
    "fast_per_droplet_setup": (False, 0, D.NO_COND_PRE, 0, "fast_per_droplet_setup", "lanes8"),
    "lean": (False, 0, 0, 0, "lean", "lanes8"),
    "lean_sorted": (False, 0, D.COND_SORTED_ORDER, 0, "lean_sorted", "direct"),
    "fold_toms748": (False, 1, 0, 0, "fold_toms748", "lanes8"),
    "lean_toms748": (False, 1, D.COND_NO_FOLD, 0, "lean_toms748", "lanes8"),
    "lean_toms748_sorted": (False, 1, D.COND_SORTED_ORDER, 0, "lean_toms748_sorted", "direct"),
    "toms748_two_pass_3": (False, 1, D.COND_TOMS_TWO_PASS, 3, "toms748_two_pass", "direct"),
    "toms748_two_pass_all": (False, 1, D.COND_TOMS_TWO_PASS, -1, "toms748_two_pass", "direct"),
    "lean_r3": (False, 0, D.COND_LEAN_R3, 0, "lean_r3", "lanes8"),
    "fold_lean": (False, 0, D.COND_FOLD, 0, "fold_lean", "lanes8"),
    "lean_wq": (False, 0, D.COND_WQ, 0, "lean_wq", "lanes8"),
    "lean_wq_cap128": (False, 0, D.COND_WQ | D.COND_WQ_CAP128, 0, "lean_wq", "lanes8"),
    "lean_resume_1": (False, 0, D.COND_BUDGET, 1, "lean", "lanes8"),
    "lean_resume_2": (False, 0, D.COND_BUDGET, 2, "lean", "lanes8"),
    "lean_finish_staged": (False, 0, D.FINISH_STAGED, 0, "lean", "lanes8"),
    "lean_sorted_finish_staged": (False, 0, D.COND_SORTED_ORDER | D.FINISH_STAGED, 0, "lean_sorted", "lanes8"),
}


def run(name, real_t, strict, solver, flags, budget, kernel, finish, sstp=1, raw=False, case=None, sample=None):
    """finish: the lgrngn.cond_finish name that the object must report after every step, or one name per step"""
    def make(oi, t):
        oi.strict_fp, oi.cond_solver, oi.dbg_flags, oi.dbg_cond_budget = strict, solver, int(flags), budget
        return h.hip_particles(oi, t)
    steps = []

    def after_step(prt):
        h.assert_mode(prt, strict, solver, kernel=kernel)
        want = finish if isinstance(finish, str) else finish[len(steps)]
        got = lgrngn.cond_finish(int(prt.state_u64("raw_cond_finish")[0])).name
        assert got == want, ("per-cell finish of step", len(steps), got, want)
        steps.append(got)
    worst = WORST.setdefault(real_t.__name__, {})
    seen = O.run_case(name, make, real_t, sstp, worst=worst, fixed_point=not strict, raw=raw, case=case, sample=sample, after_step=after_step)
    assert steps and (isinstance(finish, str) or len(steps) == len(finish)), steps
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
    # (one by one: a storage-order kernel on an object straight from init, so the finish gathers)
    run(name, real_t, False, solver, 0 if fused else D.COND_NO_FUSED_SUBSTEPS, 0, kernel, "none" if fused else "lanes8", sstp=4)


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("sstp", [1, 3])
@pytest.mark.parametrize("mode", ["api_default", "bench"])
def test_scalar_kappa_whole_steps(mode, sstp, real_t):
    """straight from init, nothing read but the raw storage: the UNI = true instantiations and the carried scatter of the production
    order.  The finish: the first step_cond finds the order that init made and carries no scatter, so its storage-order kernel leaves the
    changes to be gathered; each later one carries the scatter of the sort that step_async left to it, which puts every change at its
    droplet's place in the sorted order.  The fused substeps finish for themselves."""
    h.api_default_opts(lgrngn.opts_init_t())
    strict, solver = (h.API_DEFAULTS["strict_fp"], h.API_DEFAULTS["cond_solver"]) if mode == "api_default" else (False, 0)
    assert not strict
    kernel = "substeps" if sstp > 1 else ("lean", "fold_toms748")[solver]
    run("S", real_t, strict, solver, 0, 0, kernel, "none" if sstp > 1 else ("lanes8", "direct", "direct"), sstp=sstp, raw=True)


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
    run("C", real_t, False, 0, 0, 0, "lean", "wave", case=case, sample=rng.choice(int(counts.sum()), 20000, replace=False))
