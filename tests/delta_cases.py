"""Set-ups of the delta-transfer tests (test_delta_premise.py, test_gpu_delta.py, test_gpu_glue_delta.py): a Case with
Sneddon Dirichlet lines and some active phase-field dofs, and a second ``solution`` for the same ``old_solution`` /
``old_old_solution`` -- two Newton iterations of one time step."""
import numpy as np

import cases
import oracle_api as O
from cracks_amd import mesh as M


def with_active_phi(c: cases.Case, every: int = 5) -> cases.Case:
    """The case with every ``every``-th phase-field dof in the active set (cracks.cc:2878-2879) next to its Dirichlet lines."""
    lay, mesh = c.layout, c.mesh
    dirichlet = np.nonzero(c.cu.flag.astype(bool) & ~c.ch.flag.astype(bool))[0]
    active = lay.dof(np.arange(0, mesh.n_nodes, every), lay.dim)
    active = active[~c.ch.flag.astype(bool)[active]]
    cu = M.update_constraints(mesh, lay, dirichlet, active)
    return cases.Case(c.name + "_active", mesh, lay, c.params, c.sol, c.old, c.oldold, cu, c.ch, None, c.cell_lambda, c.cell_mu)


def box_case(dim: int, n, blocked: bool, split: bool = False, seed: int = 3) -> cases.Case:
    mesh = M.box_mesh(dim, n)
    h = mesh.min_cell_diameter()
    lay = M.DofLayout(mesh.n_nodes, dim, blocked)
    base = cases.kat_sneddon_3d(4) if dim == 3 else cases.kat_sneddon_2d()
    prm = O.PfmParams.from_buffer_copy(bytes(base.params))
    prm.alpha_eps, prm.constant_k = 2.0 * h, 1e-8 * h
    if split:
        prm.decompose_stress_matrix, prm.decompose_stress_rhs, prm.timestep_number = 1.0, 1.0, 1
    phi = M.initial_values_sneddon(mesh, h)
    sol = lay.pack(np.zeros((mesh.n_nodes, dim)), phi)
    ch = M.hanging_constraints(mesh, lay)
    cu = M.update_constraints(mesh, lay, M.sneddon_dirichlet_dofs(mesh, lay))
    c = cases.perturbed(cases.Case("box", mesh, lay, prm, sol, sol.copy(), sol.copy(), cu, ch), seed=seed)
    return with_active_phi(c)


def second_solution(c: cases.Case, seed: int = 77) -> np.ndarray:
    """Another ``solution`` for the same case: every unconstrained dof differs from ``c.sol``."""
    rng = np.random.default_rng(seed)
    node, comp = c.layout.node_comp_of_dof()
    is_phi = comp == c.layout.dim
    w = c.sol.copy()
    w[~is_phi] += rng.uniform(-1e-3, 1e-3, (~is_phi).sum())
    w[is_phi] = np.clip(w[is_phi] + rng.uniform(-0.2, 0.2, is_phi.sum()), 0.0, 1.0)
    w = c.ch.distribute(w)
    dmask = c.cu.flag.astype(bool) & ~c.ch.flag.astype(bool)
    w[dmask] = c.sol[dmask]
    return w


def displacement_rows_mask(c: cases.Case, rowptr: np.ndarray) -> np.ndarray:
    """One flag per entry of the global CSR: the entry sits in a displacement row."""
    node, comp = c.layout.node_comp_of_dof()
    return np.repeat(comp < c.layout.dim, np.diff(rowptr))
