"""numpy reference of a 3-D assembly with the volumetric-deviatoric stress split (PFM_SPLIT_VOLDEV): the element matrices
of tests/split3d_ref.py -- the statements of cracks.cc:2248-2432 -- with ``voldev_split`` / ``voldev_tangent`` of
cracks_amd/split3d.py in the place of the spectral law, and the distribution of tests/split3d_ref.py unchanged
(distribute_matrix, distribute_vector, residual_total: imported, not restated).

Same interface as split3d_ref: ``element_matrices``, ``assemble``, ``assemble_residuals``; ``trace_conditions`` gives what
the GPU tests assert of their inputs.  tests/test_split_voldev_ref_cpu.py pins this file."""
import numpy as np

import split3d_ref as R
from cracks_amd.split3d import voldev_split, voldev_tangent
from split3d_ref import distribute_matrix, distribute_vector, nodal, residual_total  # noqa: F401  (the shared distribution)


def element_matrices(mesh, lay, prm, sol, old, oldold, cell_lambda=None, cell_mu=None, split=None, jacobian=True):
    """(Ke [cell, 32, 32] or None, Re [cell, 32], E [cell, q, 3, 3]); local index = 4 * vertex + component.
    split: None = what the parameters say (decompose_stress_matrix > 0 and timestep_number > 0)."""
    assert mesh.dim == 3
    if split is None:
        split = prm.decompose_stress_matrix > 0 and prm.timestep_number > 0
    N, dN, W = R._reference_cell()
    cells = mesh.cells.astype(np.int64)
    X = mesh.coords[cells]  # [c, v, i]
    J = np.einsum("cvi,qvk->cqik", X, dN)
    det = np.linalg.det(J)
    inv = np.linalg.inv(J)  # inv[k, i] = d xi_k / d x_i
    G = np.einsum("cqkd,qvk->cqvd", inv, dN)  # grad N_v
    JxW = det * W[None, :]
    u, phi = nodal(lay, sol)
    _, phio = nodal(lay, old)
    _, phioo = nodal(lay, oldold)
    gu = np.einsum("cvi,cqvd->cqid", u[cells], G)
    pf = np.einsum("cv,qv->cq", phi[cells], N)
    pfo = np.einsum("cv,qv->cq", phio[cells], N)
    pfoo = np.einsum("cv,qv->cq", phioo[cells], N)
    gpf = np.einsum("cv,cqvd->cqd", phi[cells], G)
    mono = prm.outer_solver == 1
    gamma = 0.0 if (mono and prm.timestep_number < 1) else prm.gamma_penal
    if mono:
        pf, pfo, pfoo = np.maximum(pf, 0.0), np.maximum(pfo, 0.0), np.maximum(pfoo, 0.0)
    pf_plus = np.maximum(0.0, pf - pfo)
    t, dt, ddt = prm.time, prm.old_timestep, prm.old_old_timestep
    pfx = pfoo + (t - (t - dt - ddt)) / (t - dt - (t - dt - ddt)) * (pfo - pfoo)
    pfx = np.clip(pfx, 0.0, 1.0)
    if prm.use_old_timestep_pf:
        pfx = pfo
    kap, eps, Gc, p, aB1 = prm.constant_k, prm.alpha_eps, prm.G_c, prm.pressure, prm.alpha_biot - 1.0
    g = (1 - kap) * pfx * pfx + kap
    E = 0.5 * (gu + np.swapaxes(gu, -1, -2))
    divu = np.trace(gu, axis1=-2, axis2=-1)
    nc = cells.shape[0]
    lam = np.full(nc, prm.lambda_) if cell_lambda is None else np.asarray(cell_lambda, float)
    mu = np.full(nc, prm.mu) if cell_mu is None else np.asarray(cell_mu, float)
    lam_q, mu_q = np.broadcast_to(lam[:, None], pf.shape), np.broadcast_to(mu[:, None], pf.shape)
    I = np.eye(3)
    if split:
        sp_, sm_ = voldev_split(E, lam_q, mu_q)
    else:
        sp_ = lam_q[..., None, None] * np.trace(E, axis1=-2, axis2=-1)[..., None, None] * I + 2 * mu_q[..., None, None] * E
        sm_ = np.zeros_like(sp_)
    spE = np.einsum("cqij,cqij->cq", sp_, E)
    diam2 = np.zeros(nc)
    for v in range(4):
        diam2 = np.maximum(diam2, ((X[:, v] - X[:, 7 - v]) ** 2).sum(axis=1))
    pen = (gamma / prm.timestep / diam2)[:, None]
    # ---- residual, cracks.cc:2393-2432
    S = g[..., None, None] * sp_ + prm.decompose_stress_rhs * sm_ - (aB1 * p * pfx * pfx)[..., None, None] * I
    Ru = -np.einsum("cq,cqij,cqaj->cai", JxW, S, G)
    rphi = pen * pf_plus + (1 - kap) * spE * pf - Gc / eps * (1 - pf) - 2 * aB1 * p * pf * divu
    Rp = -(np.einsum("cq,cq,qa->ca", JxW, rphi, N) + Gc * eps * np.einsum("cq,cqd,cqad->ca", JxW, gpf, G))
    Re = np.concatenate([Ru, Rp[:, :, None]], axis=2).reshape(nc, 32)
    if not jacobian:
        return None, Re, E
    # ---- matrix, cracks.cc:2308-2389: sigma+-_LinU = C+- : E_LinU, E_LinU of trial dof (b, d) = sym(e_d (x) grad N_b)
    if split:
        Cp, Cm = voldev_tangent(E, lam_q, mu_q)
    else:
        II = np.einsum("ab,cd->abcd", I, I)
        Is = 0.5 * (np.einsum("ac,bd->abcd", I, I) + np.einsum("ad,bc->abcd", I, I))
        Cp = lam_q[..., None, None, None, None] * II + 2 * mu_q[..., None, None, None, None] * Is
        Cm = np.zeros_like(Cp)
    D = g[..., None, None, None, None] * Cp + prm.decompose_stress_matrix * Cm
    Kuu = np.einsum("cq,cqijdl,cqaj,cqbl->caibd", JxW, D, G, G)
    lin = np.einsum("cqijdl,cqij,cqbl->cqbd", Cp, E, G) + np.einsum("cqdl,cqbl->cqbd", sp_, G)  # sigma+_LinU : E + sigma+ : E_LinU
    Kpu = np.einsum("cq,qa,cqbd->cabd", JxW, N, ((1 - kap) * pf)[..., None, None] * lin - (2 * aB1 * p * pf)[..., None, None] * G)
    pen_on = np.where((pf - pfo) < 0.0, 0.0, 1.0)  # the shadowed variable of cracks.cc:2311-2315
    cpp = pen * pen_on + (1 - kap) * spE + Gc / eps - 2 * aB1 * p * divu
    Kpp = np.einsum("cq,cq,qa,qb->cab", JxW, cpp, N, N) + Gc * eps * np.einsum("cq,cqad,cqbd->cab", JxW, G, G)
    # trial phase-field dofs do not enter the displacement rows (cracks.cc:2333-2337): zeros
    Ke = np.zeros((nc, 8, 4, 8, 4))
    Ke[:, :, :3, :, :3] = Kuu
    Ke[:, :, 3, :, :3] = Kpu
    Ke[:, :, 3, :, 3] = Kpp
    return Ke.reshape(nc, 32, 32), Re, E


def assemble(mesh, lay, prm, sol, old, oldold, cell_lambda=None, cell_mu=None, split=None, jacobian=True, cu=None, ch=None):
    """as split3d_ref.assemble -> (A or None, residual_pde, E)"""
    Ke, Re, E = element_matrices(mesh, lay, prm, sol, old, oldold, cell_lambda, cell_mu, split, jacobian)
    if not jacobian:
        return None, distribute_vector(lay, mesh.cells, Re, cu), E
    A, res = distribute_matrix(mesh, lay, Ke, Re, cu)
    return A, res, E


def assemble_residuals(mesh, lay, prm, sol, old, oldold, cell_lambda=None, cell_mu=None, split=None, cu=None, ch=None):
    """as split3d_ref.assemble_residuals -> (residual_pde, residual_total, E)"""
    _, Re, E = element_matrices(mesh, lay, prm, sol, old, oldold, cell_lambda, cell_mu, split, jacobian=False)
    return distribute_vector(lay, mesh.cells, Re, cu), residual_total(lay, mesh.cells, prm, Re, cu, ch), E


def trace_conditions(E):
    """(share of the q-points with tr E > 0, min over the q-points of |tr E| / |E|_F)"""
    tr = np.trace(E, axis1=-2, axis2=-1)
    return float((tr > 0.0).mean()), float((np.abs(tr) / np.linalg.norm(E, axis=(-2, -1))).min())
