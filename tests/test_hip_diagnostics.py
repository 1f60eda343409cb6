"""The diagnostics of the HIP object, double and float, against tests/_diag_reference.py (numpy long double, written from the
reference's sources, no project code) on the crafted states of tests/test_oracle_diagnostics.py: workgroups of k_cell_seqsum at and
over the staging cap, a cell above it, cf_cells() lowered to 5 and to 1, empty cells at group edges and at the domain's end, the
knife edges of [min, max), odd moments of negative values, dead storage slots under an object nobody has read, multiplicity 0 in
the order.  The cases, the tolerances and their derivation are in that module (CASES, check)."""
import numpy as np
import pytest

import _harness as h
import test_oracle_diagnostics as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(D.CASES))
def test_hip_diagnostics_match_the_plain_reference(name, real_t):
    after = None
    if name == "A1_api_default":                           # the diagnostics must not depend on the arithmetic mode (vt is read back)
        after = lambda prt: h.assert_mode(prt, False, 1)
    D.run_case(name, h.hip_particles, real_t, after=after, raw_storage=True)
