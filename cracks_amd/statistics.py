"""The reference's statistics from the converged state of a time step, on the device (include/pfm_newton.h).

    statistics block of the time loop     cracks.cc:4436-4460  -> ``load_statistic`` (compute_load, cracks.cc:3726-3816)
    Sneddon, end of a refinement cycle    cracks.cc:4489-4524  -> ``sneddon_end_of_cycle`` (compute_tcv,
                                                                   compute_functional_values / compute_cod,
                                                                   integrate_difference against ExactPhiSneddon)
    compute_cod_array (switched off)      cracks.cc:3337-3449  -> ``Context.cod_buckets``, ``cod_array_from_sums``,
                                                                   ``cod_array_error``
    compute_point_stress / _value         cracks.cc:3264-3320  -> ``point_stress``, ``point_value``

``cod_buckets_numpy`` and ``point_eval_numpy`` are the float64 numpy statements of the two device sweeps
(``pfm_cod_buckets``, ``pfm_point_eval``): what the device entries are compared against.

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


# ---- compute_cod_array (cracks.cc:3337-3449) and the point evaluation (cracks.cc:3264-3320) -------------------------

POINT_BOX_TOL, POINT_CELL_TOL, POINT_STEP_TOL, POINT_NEWTON_STEPS = 1e-8, 1e-10, 1e-12, 20  # include/pfm_newton.h
NO_POINT_VALUE = -1e100  # compute_point_value without a cell (cracks.cc:3270)


def _q1_shape(dim: int, xi: np.ndarray):
    """Q1 values [..., nv] and reference gradients [..., nv, dim] at the points xi [..., dim]."""
    nv = 1 << dim
    N = np.ones(xi.shape[:-1] + (nv,))
    dN = np.ones(xi.shape[:-1] + (nv, dim))
    for b in range(nv):
        for d in range(dim):
            bit = (b >> d) & 1
            f = xi[..., d] if bit else 1.0 - xi[..., d]
            N[..., b] *= f
            for e in range(dim):
                dN[..., b, e] *= (1.0 if bit else -1.0) if e == d else f
    return N, dN


def _det_adj(J: np.ndarray):
    """det [...] and adjugate [..., dim, dim] (inverse * det) of J [..., dim, dim], dim 2 or 3, written out."""
    dim = J.shape[-1]
    A = np.empty_like(J)
    if dim == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        A[..., 0, 0], A[..., 0, 1], A[..., 1, 0], A[..., 1, 1] = J[..., 1, 1], -J[..., 0, 1], -J[..., 1, 0], J[..., 0, 0]
        return det, A
    for i in range(3):
        for j in range(3):
            a, b, c, d = (j + 1) % 3, (j + 2) % 3, (i + 1) % 3, (i + 2) % 3
            A[..., i, j] = J[..., a, c] * J[..., b, d] - J[..., a, d] * J[..., b, c]
    det = J[..., 0, 0] * A[..., 0, 0] + J[..., 0, 1] * A[..., 1, 0] + J[..., 0, 2] * A[..., 2, 0]
    return det, A


def value_to_bucket(x, n_buckets: int = 75, x_lo: float = -1.5, x_hi: float = 1.5):
    """``value_to_bucket`` (cracks.cc:3323-3328) before its cast, with its constants made arguments: the real number whose
    floor is the bucket, evaluated in this order."""
    return (np.asarray(x, float) - x_lo) / (x_hi - x_lo) * n_buckets + 0.5


def bucket_to_value(idx, n_buckets: int = 75, x_lo: float = -1.5, x_hi: float = 1.5):
    """``bucket_to_value`` (cracks.cc:3330-3335)."""
    return x_lo + np.asarray(idx, float) * (x_hi - x_lo) / n_buckets


def cod_buckets_numpy(mesh, nodal: np.ndarray, n_buckets: int = 75, x_lo: float = -1.5, x_hi: float = 1.5, n_sub: int = 100,
                      cell_owned: Optional[np.ndarray] = None, info: Optional[dict] = None, cells_per_chunk: int = 0):
    """``pfm_cod_buckets``: the loop of compute_cod_array (cracks.cc:3354-3410) over the cells with ``cell_owned != 0`` for
    the nodal values ``nodal`` [n_nodes, dim + 1] (displacements, then phi; hanging nodes distributed): every cell is sampled
    at the ``n_sub^dim`` midpoints ``xi_d = (k_d + 0.5) / n_sub`` (k_0 fastest) with weight ``n_sub^-dim``; ``(values,
    volume)`` = the bucket sums of ``u . grad(phi) JxW`` and ``JxW`` with MappingQ1.  ``info["tie_margin"]`` receives the
    smallest distance of ``value_to_bucket`` from an integer over all sampled points (a point closer to a bucket boundary
    than the rounding of x could fall on either side)."""
    dim, nv = mesh.dim, mesh.nv
    nodal = np.asarray(nodal, float)
    k = (np.arange(n_sub) + 0.5) / n_sub
    grids = np.meshgrid(*([k] * dim), indexing="ij")  # axis d of the grid <-> k_{dim-1-d}: k_0 fastest
    xi = np.stack([g.ravel() for g in reversed(grids)], axis=1)
    N, dN = _q1_shape(dim, xi)  # [P, nv], [P, nv, dim]
    weight = 1.0 / float(n_sub) ** dim
    own = np.arange(mesh.n_cells) if cell_owned is None else np.nonzero(np.asarray(cell_owned))[0]
    # the bucket sums are accumulated in extended precision where the platform has it: a running double sum over the 1e4
    # points of a bucket drifts by 1e-13 relative, a tenth of the bar the device sums are compared at
    values, volume = np.zeros(n_buckets, np.longdouble), np.zeros(n_buckets, np.longdouble)
    margin = np.inf
    chunk = cells_per_chunk or max(1, (1 << 19) // xi.shape[0])
    for c0 in range(0, own.size, chunk):
        cells = mesh.cells[own[c0:c0 + chunk]]
        X = mesh.coords[cells]  # [C, nv, dim]
        F = nodal[cells]  # [C, nv, dim + 1]
        x0 = X[:, :, 0] @ N.T  # [C, P]
        J = np.einsum("cbi,pbj->cpij", X, dN)
        det, adj = _det_adj(J)
        u = np.einsum("cbi,pb->cpi", F[:, :, :dim], N)
        gref = np.einsum("cb,pbe->cpe", F[:, :, dim], dN)
        # grad phi_i = sum_e inv[e, i] gref_e;  (u . grad phi) det = gref^T adj u
        ugp = np.einsum("cpe,cpei,cpi->cp", gref, adj, u) / det
        jxw = det * weight
        t = value_to_bucket(x0, n_buckets, x_lo, x_hi)
        margin = min(margin, float(np.min(np.abs(t - np.rint(t)))) if t.size else np.inf)
        idx = np.floor(t)
        keep = (idx >= 0) & (idx < n_buckets)
        ii = idx[keep].astype(np.int64)
        order = np.argsort(ii, kind="stable")
        counts = np.bincount(ii, minlength=n_buckets)
        filled = np.nonzero(counts)[0]
        starts = (np.cumsum(counts) - counts)[filled]
        if filled.size:
            for total, w in ((values, (ugp * jxw)[keep]), (volume, jxw[keep])):
                total[filled] += np.add.reduceat(w[order].astype(np.longdouble), starts)
    if info is not None:
        info["tie_margin"] = margin
    return values.astype(np.float64), volume.astype(np.float64)


def cod_array_from_sums(values_sum, n_buckets: int = 75, x_lo: float = -1.5, x_hi: float = 1.5) -> np.ndarray:
    """The three columns of ``cod-NN.txt`` (cracks.cc:3436), an array [n_buckets, 3], from the MPI-summed bucket values
    [n_buckets]: ``bucket_to_value(i)``, ``values / width / 2`` with the width of cracks.cc:3377, and the exact Sneddon profile
    ``1.92e-3 sqrt(max(0, 1 - x^2))`` (cracks.cc:3351)."""
    x = bucket_to_value(np.arange(n_buckets), n_buckets, x_lo, x_hi)
    width = float(bucket_to_value(1, n_buckets, x_lo, x_hi) - bucket_to_value(0, n_buckets, x_lo, x_hi))
    exact = 1.92e-3 * np.sqrt(np.maximum(0.0, 1.0 - x * x))
    return np.stack([x, np.asarray(values_sum, float) / width / 2.0, exact], axis=1)


def cod_array_error(columns: np.ndarray) -> float:
    """The ``ERROR:`` norm of compute_cod_array (cracks.cc:3432-3438) of the columns of ``cod_array_from_sums``."""
    return math.sqrt(float(np.sum((columns[:, 1] - columns[:, 2]) ** 2)))


def _newton_inverse(X: np.ndarray, p: np.ndarray):
    """The Newton inverse of the Q1 map of ``pfm_point_eval`` for the pairs (cell vertices X [K, nv, dim], point p [K, dim]):
    from the cell centre, at most 20 steps, converged when a step is <= 1e-12 in every coordinate; a step that is not
    finite ends the pair.  Returns (xi [K, dim], converged [K])."""
    K, _, dim = X.shape
    xi = np.full((K, dim), 0.5)
    converged = np.zeros(K, bool)
    live = np.ones(K, bool)
    for _ in range(POINT_NEWTON_STEPS):
        a = np.nonzero(live)[0]
        if a.size == 0:
            break
        N, dN = _q1_shape(dim, xi[a])
        Fv = np.einsum("kbi,kb->ki", X[a], N) - p[a]
        J = np.einsum("kbi,kbj->kij", X[a], dN)
        det, adj = _det_adj(J)
        with np.errstate(all="ignore"):
            dx = np.einsum("kij,kj->ki", adj, Fv) / det[:, None]
            xi[a] = xi[a] - dx
            finite = np.all(np.abs(dx) <= 1e300, axis=1)
            small = finite & (np.max(np.abs(dx), axis=1) <= POINT_STEP_TOL)
        converged[a[small]] = True
        live[a[small | ~finite]] = False
    return xi, converged


def point_eval_numpy(mesh, nodal: np.ndarray, points, cell_owned: Optional[np.ndarray] = None):
    """``pfm_point_eval`` for the nodal values ``nodal`` [n_nodes, dim + 1]: ``(cell, values, grads)``.  ``cell[p]`` is the
    LOWEST-numbered masked cell whose Newton inverse of the Q1 map converges to a xi in ``[-1e-10, 1 + 1e-10]^dim``, tried only
    for the cells whose vertex bounding box, inflated by 1e-8 cell diameters, holds the point; -1 without one (values and
    gradients 0).  The evaluation clamps xi to the unit cell; ``grads[p, c, d] = d(component c)/dx_d``.
    Asserts that no candidate's overshoot beyond the unit cell lies in (1e-11, 1e-9): the decisions are then safe against
    the rounding of another evaluation order."""
    dim, nv = mesh.dim, mesh.nv
    nodal = np.asarray(nodal, float)
    pts = np.asarray(points, float).reshape(-1, dim)
    P = pts.shape[0]
    own = np.arange(mesh.n_cells) if cell_owned is None else np.nonzero(np.asarray(cell_owned))[0]
    Xall = mesh.coords[mesh.cells[own]]
    tol = POINT_BOX_TOL * mesh.cell_diameters()[own]
    lo, hi = Xall.min(axis=1) - tol[:, None], Xall.max(axis=1) + tol[:, None]
    cell = np.full(P, -1, np.int32)
    values, grads = np.zeros((P, dim + 1)), np.zeros((P, dim + 1, dim))
    xi_of = np.zeros((P, dim))
    step = max(1, (1 << 22) // max(own.size, 1))
    for p0 in range(0, P, step):
        pp = pts[p0:p0 + step]
        inside = np.all((pp[:, None, :] >= lo[None]) & (pp[:, None, :] <= hi[None]), axis=2)
        pi, ci = np.nonzero(inside)  # sorted by point, then ascending cell
        if pi.size == 0:
            continue
        xi, ok = _newton_inverse(Xall[ci], pp[pi])
        over = np.maximum(np.max(-xi, axis=1), np.max(xi - 1.0, axis=1))
        assert not np.any(ok & (over > 1e-11) & (over < 1e-9)), "a candidate cell within rounding of the cell tolerance"
        good = ok & (over <= POINT_CELL_TOL)
        for k in np.nonzero(good)[0][::-1]:  # descending: the lowest cell of a point is written last
            cell[p0 + pi[k]] = own[ci[k]]
            xi_of[p0 + pi[k]] = xi[k]
    has = np.nonzero(cell >= 0)[0]
    if has.size:
        xc = np.clip(xi_of[has], 0.0, 1.0)  # project_to_unit_cell
        X, F = mesh.coords[mesh.cells[cell[has]]], nodal[mesh.cells[cell[has]]]
        N, dN = _q1_shape(dim, xc)
        J = np.einsum("kbi,kbj->kij", X, dN)
        det, adj = _det_adj(J)
        g = np.einsum("kej,kbe->kbj", adj / det[:, None, None], dN)  # physical shape gradients
        values[has] = np.einsum("kbc,kb->kc", F, N)
        grads[has] = np.einsum("kbc,kbj->kcj", F, g)
    return cell, values, grads


def point_stress_from_eval(cell, grads) -> float:
    """compute_point_stress (cracks.cc:3302-3316) from the evaluation of its one point: ``-d u_y / d y``, 0.0 without a
    cell (a partitioned caller takes the maximum over the ranks, cracks.cc:3319)."""
    return -float(grads[0][1][1]) if int(cell[0]) >= 0 else 0.0


def point_stress(ctx, point=(0.0, 2.0), cell_owned: Optional[np.ndarray] = None) -> float:
    """The ``PStress:`` number of the three-point bending statistics (cracks.cc:3285-3320) on the device."""
    cell, _, grads = ctx.point_eval([point], cell_owned)
    return point_stress_from_eval(cell, grads)


def point_value(ctx, point, component: int, cell_owned: Optional[np.ndarray] = None) -> float:
    """compute_point_value (cracks.cc:3264-3283) on the device: the component at the point, -1e100 without a cell (the
    caller takes the maximum over the ranks)."""
    cell, values, _ = ctx.point_eval([point], cell_owned)
    return float(values[0][component]) if int(cell[0]) >= 0 else NO_POINT_VALUE
