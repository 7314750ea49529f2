"""The premise of the delta transfer ("Delta transfer"), on the CPU oracle: within a time step -- same
old_solution / old_old_solution, constraints and parameters -- the displacement rows of the Jacobian do not depend on
``solution`` unless the stress split is on (cracks.cc:2262-2277, 2356-2364: they see the phase field only through the
lagged extrapolation).  Two solutions, bitwise comparison of the oracle's matrix values; with the 2-D split on the rows
do change.  pfm_values_to_host_delta does not rely on this (it compares); this documents why it pays."""
import numpy as np
import pytest

from cracks_amd import mesh as M
import oracle_api as O
from delta_cases import box_case, displacement_rows_mask, second_solution


def _two_matrices(c):
    rp, ci = M.dof_sparsity(c.mesh, c.layout)
    out = []
    for sol in (c.sol, second_solution(c)):
        r = O.assemble(c.mesh, c.layout, c.params, sol, c.old, c.oldold, c.cu, c.ch, False, rp, ci)
        assert r.err == 0
        out.append(np.array(r.values, copy=True))
    return out[0], out[1], displacement_rows_mask(c, rp)


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("dim,n", [(3, (5, 4, 3)), (2, (7, 6))])
def test_displacement_rows_do_not_depend_on_the_solution(dim, n, blocked):
    a, b, urow = _two_matrices(box_case(dim, n, blocked))
    assert urow.any() and not urow.all()
    # bit for bit, the placeholder diagonals of constrained rows included
    assert np.array_equal(a[urow].view(np.uint64), b[urow].view(np.uint64))
    # ... while the phase-field rows do change: the two solutions are different inputs
    assert (a[~urow].view(np.uint64) != b[~urow].view(np.uint64)).any()


@pytest.mark.parametrize("blocked", [True, False])
def test_with_the_stress_split_the_displacement_rows_change(blocked):
    a, b, urow = _two_matrices(box_case(2, (7, 6), blocked, split=True))
    assert (a[urow].view(np.uint64) != b[urow].view(np.uint64)).any()
