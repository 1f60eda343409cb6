"""The move of the HIP object -- k_move in its nine instantiations, the fused re-indexing, the puddle's reduction, hskpng_ijk -- double and
float, strict_fp 1 and 0, against tests/_move_reference.py (numpy long double, written from the reference's sources, no project code) on
the crafted cases of tests/test_oracle_move.py: the exact box (bit for bit), the rounding box under euler, implicit and pred_corr, the
predictor-corrector's fallback, clamps and y shift, the switches, a slab with neighbours.  The cases, the checks and the bars (measured
on the CPU oracle, never here) are in that module; WORST collects what the device reaches, for the record.

Every case runs by single stages (adve, sedi, bcnd, hskpng_ijk: the generic, MOVE_3D and predictor-corrector kernels one operation at a
time, each held to the reference started from what the stage before stored) and as a whole step_async (the fused re-indexing, the
MOVE_FULL kernels, the turbulent ones).  Which instantiation ran is read back ("raw_move_kernel") behind every launch and held to what
lcx_core.hip's move() is meant to choose (test_oracle_move.expected_kernel); the last test makes one run per instantiation and lists the set."""
import numpy as np
import pytest

import _harness as h
import test_oracle_move as O

pytestmark = pytest.mark.gpu

WORST = {}
MODES = [(np.float64, True), (np.float64, False), (np.float32, True), (np.float32, False)]
MODE_IDS = ["f64-strict", "f64-fast", "f32-strict", "f32-fast"]


def run(name, real_t, strict, staged):
    def make(oi, t):
        oi.strict_fp = strict
        return h.hip_particles(oi, t)

    def saw(prt, case, step, stage):
        got = prt.move_kernel()
        assert got == O.expected_kernel(case, step, stage), (name, step, stage, got, O.expected_kernel(case, step, stage))
        h.assert_mode(prt, strict)
        seen_here.append(got)
    seen_here = []
    worst = WORST.setdefault((real_t.__name__, strict), {})
    fates = O.run_case(name, make, real_t, staged, prefix="raw_", worst=worst, eps_acc=np.finfo(np.float64).eps, saw_kernel=saw, counts_dead_migrants=False)
    assert seen_here, "every test reads the kernel back"
    print("\nhip move %s %s %s strict_fp %d: kernels %s MEASURED so far %s oracle's worst %s bars %s fates %s"
          % (name, "staged" if staged else "whole", real_t.__name__, strict, sorted(set(seen_here)), {k: round(v, 3) for k, v in worst.items()},
             O.MEASURED[real_t], O.BARS[real_t], fates))
    return set(seen_here)


@pytest.mark.parametrize("real_t,strict", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", O.STAGED)
def test_stages(name, real_t, strict):
    run(name, real_t, strict, True)


@pytest.mark.parametrize("real_t,strict", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(O.CASES))
def test_whole_step(name, real_t, strict):
    run(name, real_t, strict, False)


def test_all_nine_instantiations_are_read_back():
    """one run per k_move that move() can launch (test_oracle_move.planned_kernels: which case reaches which), made here, so that the set
    does not depend on which other tests ran: what the object reported is the nine, no more and no fewer"""
    seen = set()
    for kernel, (name, staged) in sorted(O.planned_kernels().items()):
        got = run(name, np.float64, True, staged)
        assert kernel in got, (kernel, name, staged, got)
        seen |= got
    print("\nk_move instantiations read back (PC, TURB, SPEC):", sorted(seen))
    assert seen == O.NINE, sorted(seen ^ O.NINE)
