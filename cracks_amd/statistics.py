"""The reference's statistics from the converged state of a time step, on the device (include/pfm_newton.h).

    statistics block of the time loop     cracks.cc:4436-4460  -> ``load_statistic`` (compute_load, cracks.cc:3726-3816)
    Sneddon, end of a refinement cycle    cracks.cc:4489-4524  -> ``sneddon_end_of_cycle`` (compute_tcv,
                                                                   compute_functional_values / compute_cod,
                                                                   integrate_difference against ExactPhiSneddon)

The library returns this rank's raw sums; what the reference does after them -- the MPI sum, the sign flips of
compute_load, the ``/2`` and the ``-1e300`` of compute_cod, the root of the phi error -- is done here, on the summed
values (``*_from_sums``), so that a partitioned caller adds the ranks' raw outputs first and then calls the same
functions.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

MIEHE_SHEAR, MIEHE_TENSION, THREE_POINT = "miehe_shear", "miehe_tension", "three_point_bending"
LOAD_NAMES = {MIEHE_SHEAR: "Load x", MIEHE_TENSION: "Load y", THREE_POINT: "Load P11"}
COD_EPS = 1.0e-8  # compute_cod, cracks.cc:3477
NO_FACES = -1e300  # compute_cod's value of a line no face matched (cracks.cc:3541-3543)


def cod_lines(n: int = 16 * 16) -> np.ndarray:
    """The evaluation lines of compute_functional_values (cracks.cc:3716-3720): x_i = -1.5 + i * (1.0 / N), i = 0 .. 3N,
    computed in the same order of operations."""
    dx = 1.0 / n
    return np.array([-1.5 + i * dx for i in range(3 * n + 1)])


def load_from_sums(test_case: str, raw: Sequence[float]) -> float:
    """The printed load of compute_load (cracks.cc:3792-3815) from the summed raw vector int sigma n: the x component is
    negated for every case; shear prints it, tension prints the (unflipped) y component, three-point the negated y."""
    if test_case == MIEHE_SHEAR:
        return -float(raw[0])
    if test_case == MIEHE_TENSION:
        return float(raw[1])
    if test_case == THREE_POINT:
        return -float(raw[1])
    raise ValueError(f"compute_load has no statistic for test case {test_case!r}")


def load_statistic(ctx, test_case: str, cells, faces) -> float:
    """compute_load of one rank's (cell, face) list (boundary id 3 of its owned cells) on the device."""
    return load_from_sums(test_case, ctx.face_load(cells, faces))


def cod_from_sums(cod_sum, n_faces_sum) -> np.ndarray:
    """compute_cod after its MPI sums (cracks.cc:3538-3543): value / 2 (each face is counted from both of its cells), and
    -1e300 for a line without faces."""
    cod_sum = np.asarray(cod_sum, float)
    return np.where(np.asarray(n_faces_sum) == 0, NO_FACES, cod_sum / 2.0)


def tcv_exact(dim: int, pressure: float, nu: float, E: float = 1.0, l0: float = 1.0) -> float:
    """The ``exact=`` value compute_tcv prints next to the TCV (cracks.cc:3592-3602)."""
    if dim == 2:
        return 2.0 * pressure * l0 * l0 * (1.0 - nu * nu) * math.pi / E
    return 16.0 * pressure * l0 * l0 * l0 * (1.0 - nu * nu) / E / 3.0


def phi_l2_error_from_sums(sum_sq: float) -> float:
    """sqrt of the summed int (phi_h - phi_exact)^2 (cracks.cc:4518-4519)."""
    return math.sqrt(sum_sq)


def sneddon_end_of_cycle(ctx, pressure: float, nu: float, cell_owned: Optional[np.ndarray] = None,
                         lines: Optional[np.ndarray] = None) -> Dict[str, object]:
    """The Sneddon block once the time loop has converged (cracks.cc:4489-4524) for a single context: TCV and its exact
    value, the COD of every line that has faces (what compute_functional_values writes, line -> value) and the phi L2
    error.  The context must hold the converged state (``state_set_*``) and the current parameters."""
    lines = cod_lines() if lines is None else np.asarray(lines, float)
    tcv = ctx.functionals(cell_owned)[2]
    cod, n_faces = ctx.cod_lines(lines, cell_owned, COD_EPS)
    values = cod_from_sums(cod, n_faces)
    return {
        "tcv": tcv,
        "tcv_exact": tcv_exact(ctx.dim, pressure, nu),
        "cod": {float(x): float(v) for x, v in zip(lines, values) if v > -1e100},
        "phi_L2_error": phi_l2_error_from_sums(ctx.sneddon_phi_error_sq(cell_owned)),
    }
