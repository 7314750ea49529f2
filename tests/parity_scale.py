"""The parity bar at the scale of each block, entry, row and residual part.  A plain helper module (no fixtures, no hooks).

The project's bar is |x - x_ref| < 1e-12 * scale.  gpu_util.linf_scaled takes one scale, max(1, |x_ref|_inf), for a whole
matrix or vector.  The blocks of this system differ by up to seven orders of magnitude ((u,u) ~ 1e5, (phi,phi) ~ 1 on the
Miehe cases), so that bar says little about the small blocks: the (phi,phi) block of miehe_shear_1 rounded to float32 passes
it (tests/test_parity_scale_cpu.py lists what it accepts).  The four checks below keep the tolerance and change the scale.

Matrix, per entry     |a_ij - ref_ij| <= TOL * s_ij,  s_ij = sqrt(|d_i| |d_j|),  d = diag(A_ref).
                      (u,u) and (phi,phi) are Gram forms (Cauchy-Schwarz); the (phi,u) coupling obeys the same bound through
                      sigma:eps(N) <= sqrt(2 psi) sqrt(eps:C:eps).  The precondition |ref_ij| <= (1 + 1e-12) s_ij is a CPU
                      test on the states of GPU_CASES there.  Where s_ij = 0 in the structurally zero (u,phi) block the values
                      must be equal; any other entry with s_ij = 0 has no per-entry scale (entry_error: where and why).
Matrix, per block     uu, phiu, phiphi and uphi apart (rows and columns classified by layout.node_comp_of_dof()):
                      |a - ref|_inf <= TOL * |ref|_inf over the block's stored entries, no floor of 1; a block whose
                      reference is all zero (the structurally zero (u,phi) block) must be equal.
Residual, per row     |r_i - ref_i| <= TOL * s_i,  s_i = sum_j (|A_ij| + |A_ji|) w_j,  w_j = |sol_j| on displacement dofs and
                      1 on phase-field dofs (componentwise, Oettli-Prager).  s_i = 0: equal.  A is the reference matrix
                      whose rows belong to the vector: for residual_total of the active-set scheme (outer_solver 0), which
                      is distributed with the hanging-node constraints alone, that is the oracle's Jacobian with those
                      constraints in the place of constraints_update (gpu_util.total_matrix).
Residual, per part    u rows and phi rows apart, each at its own |ref|_inf, no floor; a part whose reference is zero: equal.

Every assertion prints what it measured (pytest -s); tests/PARITY_SCALES.md holds the largest value per test file.

No entry has a floor of its own: the references agree with each other within 1e-13 on all four checks on every case tried
(tests/test_parity_scale_cpu.py: at most 4.2e-15), so every entry is held to TOL.  Should a reference's own closed form ever
lose digits at an entry (cancellation, as in the 2-D eigen-decomposition near equal eigenvalues), the bar for that entry is
the reference's measured error against a high-precision evaluation, the kernel held to 4 times that (hardware-estimate
roots carry up to 2 ulp against 0.5 ulp for sqrt and division), with the evidence as a CPU test -- to be added to
assert_matrix then; there is no table to fill in silently."""
from __future__ import annotations

import os

import numpy as np
import scipy.sparse as sp

TOL = 1e-12
BLOCKS = ("uu", "uphi", "phiu", "phiphi")


def where():
    t = os.environ.get("PYTEST_CURRENT_TEST", "")
    return t.split("::")[0].rsplit("/", 1)[-1] if t else "-"


def report(check, tag, value):
    print(f"parity_scale [{where()}] {check:<9s} {value:9.2e}  {tag}")


def ratio(err, scale):
    """max err / scale; where scale == 0 any difference counts as infinite"""
    err, scale = np.asarray(err, float), np.asarray(scale, float)
    if err.size == 0:
        return 0.0
    out = np.zeros_like(err)
    pos = scale > 0.0
    out[pos] = err[pos] / scale[pos]
    out[~pos & (err != 0.0)] = np.inf
    out[np.isnan(err)] = np.inf
    return float(out.max())


def entry_error(got, ref, s, structurally_zero=False):
    """max |got - ref| / s over the entries that have a per-entry scale -> (error, number of entries without one).
    structurally_zero (flag or mask per entry): the entry lies in the (u,phi) block, which the assembly never writes a non-zero
    into -- there s = 0 means equal, inf otherwise.  Any other entry with s = 0 has no per-entry scale: the diagonal of its row
    or column vanishes in the reference (kappa = 0 and g = 0 in whole cells, the 'dead zones' of tests/test_gpu_cart.py; zero
    strain and G_c = 0, the 'flat' state of tests/test_gpu_overlap_phases.py) while the entry itself need not: the (phi,u)
    coupling (1 - kappa) phi sigma:eps(N_j) N_i and the pressure term 2 p phi N_i dN_j do not carry g, so the precondition
    |ref_ij| <= s_ij fails AT THAT ENTRY, and where such a sum cancels to 0.0 in the reference it does so by the order of
    its terms, not by structure.  Equality cannot be asked there: the references do not give it to each other
    (tests/test_parity_scale_cpu.py::test_entries_without_a_scale_are_those_next_to_a_vanishing_diagonal).  These entries stay under the per-block check and
    the older whole-matrix check."""
    got, ref, s = np.asarray(got, float), np.asarray(ref, float), np.asarray(s, float)
    no_scale = (s == 0.0) & ~np.broadcast_to(np.asarray(structurally_zero, bool), s.shape)
    return ratio(np.abs(got - ref)[~no_scale], s[~no_scale]), int(no_scale.sum())


def is_phi(layout):
    return layout.node_comp_of_dof()[1] == layout.dim


def _canonical(A):
    A = sp.csr_matrix(A)
    if not A.has_sorted_indices:
        A = A.copy()
        A.sort_indices()
    return A


def on_pattern(B, A):
    """B's values on A's stored pattern (B may store other zeros, or fewer); B must hold no non-zero outside it"""
    A, B = _canonical(A), sp.csr_matrix(B)
    vals = np.asarray(B[entry_rows(A), A.indices]).ravel()
    assert B.count_nonzero() == np.count_nonzero(vals), "the reference has non-zeros outside the pattern"
    return sp.csr_matrix((vals, A.indices, A.indptr), shape=A.shape)


def entry_rows(A):
    return np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))


def entry_scale(A_ref):
    """s_ij per stored entry of the reference CSR"""
    A_ref = _canonical(A_ref)
    d = np.abs(A_ref.diagonal())
    return np.sqrt(d[entry_rows(A_ref)] * d[A_ref.indices])


def block_of_entries(layout, rows, cols):
    """0 uu, 1 uphi, 2 phiu, 3 phiphi for (row, col) pairs of global dofs"""
    phi = is_phi(layout)
    return 2 * phi[rows].astype(int) + phi[cols].astype(int)


def block_error(a, ref):
    """|a - ref|_inf / |ref|_inf with no floor (ref all zero: 0 if equal, else inf)"""
    a, ref = np.asarray(a, float), np.asarray(ref, float)
    if ref.size == 0:
        return 0.0
    d, m = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    if not np.isfinite(d):
        return float("inf")
    if m > 0.0:
        return d / m
    return 0.0 if d == 0.0 else float("inf")


def matrix_errors(A, A_ref, layout):
    """(per-entry error, {block: per-block error}) of a CSR with the reference's pattern"""
    A, A_ref = _canonical(A), _canonical(A_ref)
    assert A.nnz == A_ref.nnz and (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all(), "pattern"
    blk = block_of_entries(layout, entry_rows(A_ref), A_ref.indices)
    e_entry, _ = entry_error(A.data, A_ref.data, entry_scale(A_ref), blk == 1)
    return e_entry, {BLOCKS[b]: block_error(A.data[blk == b], A_ref.data[blk == b]) for b in range(4)}


def assert_matrix(A, A_ref, layout, tol=TOL, tag=""):
    e_entry, e_block = matrix_errors(A, A_ref, layout)
    A_c = _canonical(A_ref)
    n = int(((entry_scale(A_c) == 0.0) & (block_of_entries(layout, entry_rows(A_c), A_c.indices) != 1)).sum())
    report("entry", tag + (f" ({n} entries without a per-entry scale)" if n else ""), e_entry)
    report("block", tag + " " + " ".join(f"{k}={v:.2e}" for k, v in e_block.items()), max(e_block.values()))
    assert e_entry <= tol, (tag, "per entry", e_entry)
    assert max(e_block.values()) <= tol, (tag, "per block", e_block)
    return e_entry, e_block


def cauchy_schwarz(A_ref):
    """max |ref_ij| / s_ij over the stored entries (the precondition of the per-entry scale)"""
    A_ref = _canonical(A_ref)
    return ratio(np.abs(A_ref.data), entry_scale(A_ref))


def residual_scale(A_ref, layout, sol):
    A_ref = _canonical(A_ref)
    w = np.where(is_phi(layout), 1.0, np.abs(np.asarray(sol, float)))
    B = abs(A_ref)
    return B @ w + B.T @ w


def part_errors(r, r_ref, phi_mask):
    """{part: |r - ref|_inf / |ref|_inf} over the u rows and the phi rows of the given vectors"""
    r, r_ref = np.asarray(r), np.asarray(r_ref)
    return {"u": block_error(r[~phi_mask], r_ref[~phi_mask]), "phi": block_error(r[phi_mask], r_ref[phi_mask])}


def assert_parts(r, r_ref, phi_mask, tol=TOL, tag=""):
    """Per-part check alone: for vectors (or row samples) whose reference matrix is not at hand.  phi_mask: per row."""
    e = part_errors(r, r_ref, np.asarray(phi_mask, bool))
    report("part", tag + " " + " ".join(f"{k}={v:.2e}" for k, v in e.items()), max(e.values()))
    assert max(e.values()) <= tol, (tag, "per part", e)
    return e


def assert_blocks(values, ref_values, tol=TOL, tag="", names=None):
    """Per-block check alone on value arrays that each belong to one block (or to one path's whole output, when nothing
    finer is at hand): every array at its own |ref|_inf, no floor."""
    e = {(names[k] if names else str(k)): block_error(a, b) for k, (a, b) in enumerate(zip(values, ref_values))}
    report("block", tag + " " + " ".join(f"{k}={v:.2e}" for k, v in e.items()), max(e.values()) if e else 0.0)
    assert not e or max(e.values()) <= tol, (tag, "per block", e)
    return e


def residual_errors(r, r_ref, A_ref, layout, sol):
    e_row = ratio(np.abs(np.asarray(r) - np.asarray(r_ref)), residual_scale(A_ref, layout, sol))
    return e_row, part_errors(r, r_ref, is_phi(layout))


def assert_residual(r, r_ref, A_ref, layout, sol, tol=TOL, tag=""):
    e_row, e_part = residual_errors(r, r_ref, A_ref, layout, sol)
    report("row", tag, e_row)
    report("part", tag + " " + " ".join(f"{k}={v:.2e}" for k, v in e_part.items()), max(e_part.values()))
    assert e_row <= tol, (tag, "per row", e_row)
    assert max(e_part.values()) <= tol, (tag, "per part", e_part)
    return e_row, e_part


def assert_rank_block(got, want, d_ref, grow, gcol, name, tol=TOL, tag=""):
    """One block's values of a rank (or a sample of them) whose entries are the global entries (grow, gcol): per entry with
    d_ref = |diagonal| of the global reference matrix over the global dofs, and the block at its own |want|_inf."""
    got, want, d_ref = np.asarray(got, float), np.asarray(want, float), np.abs(np.asarray(d_ref, float))
    e, _ = entry_error(got, want, np.sqrt(d_ref[grow] * d_ref[gcol]), name == "uphi")
    report("entry", f"{tag} {name}", e)
    assert e <= tol, (tag, name, "per entry", e)
    assert_blocks([got], [want], tol, tag, [name])


def assert_rank_rows(v, want, A_ref, layout, sol, gdofs, tol=TOL, tag=""):
    """Rows of a rank that are the global rows gdofs (want = the reference vector at gdofs): per row with the scale of the
    global reference matrix, per part at the parts' own |want|_inf."""
    e = ratio(np.abs(np.asarray(v) - np.asarray(want)), residual_scale(A_ref, layout, sol)[gdofs])
    report("row", tag, e)
    assert e <= tol, (tag, "per row", e)
    assert_parts(v, want, is_phi(layout)[gdofs], tol, tag)
