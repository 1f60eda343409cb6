"""Terminal velocities, collision kernels, the pair probability with its scale factor and collide() of the HIP object, in float64 and float32, with
strict_fp 1 and 0, against tests/_vterm_coal_reference.py (numpy long double, written from the reference's sources, no project code).
The cases, how a kernel value is read off the object, the tolerances and how they were measured on the CPU oracle are in
tests/test_oracle_vterm_coal.py (CASES, run_case, MEASURED -> BARS); the fast arithmetic is held to the same bars.

Which velocity kernel ran is not read back: by the host code of hskpng_vterm (lcx_core.hip) beard77 / beard77fast take
k_vterm_b77<FAST = !strict_fp, TABLE>, the other formulas k_vterm, and the refresh between coalescence substeps rank_vt_fix -- the tests
pick the options that lead there, nothing more.  The coalescence variant IS read back.  Every coalescence case runs twice: with a replayed random stream (the generic k_coal; col[] is then checked too) and without one --
for the tabulated kernels through a whole step_async, which is the production variant k_coal<T, false, true>.  Which variant ran is
read back from the object ("raw_coal_kernel": 0 generic, 1 Onishi, 2 production).

Worst deviation of the device from the long-double reference, in eps of its type, next to the bar it was held to: see the table in
DESIGN.md section 2."""
import numpy as np
import pytest

import _harness as h
import _vterm_coal_reference as R
import test_oracle_vterm_coal as V

pytestmark = pytest.mark.gpu

MODES = [(np.float64, 1), (np.float64, 0), (np.float32, 1), (np.float32, 0)]
MODE_IDS = ["f64-strict", "f64-fast", "f32-strict", "f32-fast"]


def maker(strict_fp):
    def make(oi, real_t):
        oi.strict_fp = bool(strict_fp)
        prt = h.hip_particles(oi, real_t)
        h.assert_mode(prt, strict_fp)
        return prt
    return make


def coal_kernel(prt):
    return int(prt.state_u64("raw_coal_kernel")[0])


@pytest.mark.parametrize("real_t,strict_fp", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(V.VT_CASES))
def test_hip_velocities_match_the_plain_reference(name, real_t, strict_fp):
    V.run_case(name, maker(strict_fp), real_t)


@pytest.mark.parametrize("real_t,strict_fp", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(V.COAL_CASES))
def test_hip_coalescence_replayed_matches_the_plain_reference(name, real_t, strict_fp):
    """the generic kernel on a replayed stream: the shuffle keys pushed here decide which droplet of a cell is the pair's first, so
    col[p] (the count) and col[p + 1] (-2: the first had the larger or an equal multiplicity, -1: the second) are known"""
    rng = np.random.default_rng(17)
    keys = {}

    def before_coal(prt):
        n = prt.n_part
        keys["un"] = rng.integers(0, 2 ** 32, n).astype(np.float64)
        prt.rng_replay_push(1, keys["un"])
        prt.rng_replay_push(0, rng.random(n))

    def after_coal(prt, before):
        onishi = name.startswith("onishi")
        assert coal_kernel(prt) == (1 if onishi else 0)
        col = prt.state_real("col")
        n0, n1 = before["n"], prt.state_u64("n").reshape(before["n"].shape)
        un = keys["un"].reshape(n0.shape)
        for c in range(n0.shape[0]):
            first = 0 if un[c, 0] <= un[c, 1] else 1               # (a stable sort by the key: the lower id first on a tie)
            changed = (n1[c] != n0[c]).any()
            if not changed:
                assert col[2 * c] == 0, (name, "pair", c)
                continue
            big = int(np.nonzero(n1[c] != n0[c])[0][0])
            cnt = (int(n0[c, big]) - int(n1[c, big])) // int(n0[c, 1 - big])
            assert col[2 * c] == real_t(cnt), (name, "pair", c, col[2 * c], cnt)
            assert col[2 * c + 1] == (-2 if n0[c, first] >= n0[c, 1 - first] else -1), (name, "pair", c, col[2 * c + 1])
    V.run_case(name, maker(strict_fp), real_t, before_coal=before_coal, after_coal=after_coal)


@pytest.mark.parametrize("real_t,strict_fp", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(V.COAL_CASES))
def test_hip_coalescence_own_stream_matches_the_plain_reference(name, real_t, strict_fp):
    """no replayed stream: the object's own random numbers, no col[].  A tabulated kernel goes through step_async, where the
    production variant runs; the others through the stage (the production variant is compiled for the tabulated kernels only)."""
    tabulated = name.split("/")[0] in R.TABULATED
    want = 2 if tabulated else 1 if name.startswith("onishi") else 0

    def after_coal(prt, before):
        assert coal_kernel(prt) == want, (name, coal_kernel(prt), want)
    V.run_case(name, maker(strict_fp), real_t, via="step" if tabulated else "stage", after_coal=after_coal)


@pytest.mark.parametrize("real_t,strict_fp", MODES, ids=MODE_IDS)
def test_hip_scale_factor(real_t, strict_fp):
    prt = V.run_scl(maker(strict_fp), real_t, order="raw_sorted_id")     # (the order as the stage left it, not re-ranked)
    assert coal_kernel(prt) == 0


@pytest.mark.parametrize("real_t,strict_fp", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("formula", ["beard77fast", "beard76"])
def test_hip_two_substeps(formula, real_t, strict_fp):
    """sstp_coal = 2: the grown droplets' velocities are refreshed between the substeps (by the host code's reading, inside the in-cell
    ranking of the second; not read back)"""
    prt = V.run_substeps(maker(strict_fp), real_t, formula)
    assert coal_kernel(prt) == 0                                # (with substeps a used-up droplet stays in its cell: the generic kernel)


@pytest.mark.parametrize("real_t,strict_fp", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("formula", V.ANCHOR_FORMULAS + ("beard77fast",))
def test_hip_meets_gunn_and_kinzer(formula, real_t, strict_fp):
    V.run_anchors(maker(strict_fp), real_t, formula)


@pytest.mark.parametrize("real_t,strict_fp", MODES, ids=MODE_IDS)
def test_hip_drops_a_used_up_droplet_at_the_next_step(real_t, strict_fp):
    case, prt, (before, after) = V.run_case("collide", maker(strict_fp), real_t)
    used = int((after["n"] == 0).sum())
    assert used >= 3
    opts = V.coal_opts(case)
    opts.coal = False
    prt.step_async(opts)
    assert prt.n_part == after["n"].size - used
