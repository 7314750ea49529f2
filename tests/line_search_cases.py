"""Set-ups of the line-search tests (test_gpu_line_search.py, test_gpu_glue_line_search.py): a Case, a Newton update for it
whose damped trials have strictly falling residual norms, and the composition of today's entries that
``pfm_line_search_device`` must equal."""
import numpy as np

import cases
import topology_cases as T
from delta_cases import box_case

DAMPING = 0.6


def newton_update(c: cases.Case, seed: int = 5, u_amp: float = 2e-2, phi_amp: float = 0.5) -> np.ndarray:
    """A large random perturbation as the update: zero on the lines of constraints_update, hanging nodes distributed.  The
    residual of ``c.sol + 0.6^k update`` falls with k for k = 0, 1, 2 in both norms (checked with the oracle when these
    cases were written; the GPU tests assert it on what they measure)."""
    rng = np.random.default_rng(seed)
    node, comp = c.layout.node_comp_of_dof()
    is_phi = comp == c.layout.dim
    u = np.where(is_phi, rng.uniform(-phi_amp, phi_amp, c.layout.n_dofs), rng.uniform(-u_amp, u_amp, c.layout.n_dofs))
    u[c.cu.flag.astype(bool)] = 0.0
    return c.ch.distribute(u)


# name -> (maker, bitwise, norm, restore): both norms and both restore modes are spread over the contexts
LOOP_CASES = {
    "box3d_333_blocked": (lambda: box_case(3, (3, 3, 3), True), True, "l2", "saved"),
    "box3d_322_interleaved": (lambda: box_case(3, (3, 2, 2), False), True, "linf", "subtract"),
    "box2d_12x12_blocked": (lambda: box_case(2, (12, 12), True), True, "l2", "subtract"),
    "sneddon_2d_hanging": (lambda: cases.perturbed(cases.kat_sneddon_2d()), False, "linf", "saved"),
    "hang3d": (lambda: T.make_case("hang3d", T.hang3d_mesh()), False, "l2", "saved"),
}


def compose(ctx, sol, upd, pde, tot, saved, reference, max_steps, damping, norm, restore):
    """The loop from today's entries on device tensors: advance / retreat, assemble_nl_residual_device, residual_norms.
    Returns (steps, accepted, norms of the last trial, the trial value of every trial)."""
    trials, n = [], None
    for step in range(max_steps):
        if step == 0:
            ctx.line_search_advance(sol.data_ptr(), upd.data_ptr(), saved.data_ptr() if restore == "saved" else 0)
        else:
            ctx.line_search_retreat(restore, damping, sol.data_ptr(), upd.data_ptr(), saved.data_ptr(), advance=True)
        ctx.assemble_nl_residual_device(sol.data_ptr(), pde.data_ptr(), tot.data_ptr())
        n = ctx.residual_norms(pde.data_ptr())
        trials.append(n[0] if norm == "l2" else n[1])
        if trials[-1] < reference:
            return step, True, n, trials
    ctx.line_search_retreat(restore, damping, sol.data_ptr(), upd.data_ptr(), saved.data_ptr(), advance=False)
    return max_steps, False, n, trials
