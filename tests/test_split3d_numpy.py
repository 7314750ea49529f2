"""cracks_amd/split3d.py -- the 3-D spectral stress split in numpy -- checked on its own:

* embedded planar tensors [[E2, 0], [0, 0]] reproduce the reference's 2-D closed form (oracle_decompose_stress_2d, both
  branches) in their in-plane entries;
* spectral_tangent is the derivative of spectral_split (central differences);
* neither function depends on the basis chosen inside a repeated eigenspace.
"""
import numpy as np
import pytest

import oracle_api as O
from cracks_amd.split3d import positive_part, spectral_split, spectral_tangent

LAM, MU = 121.15, 80.77
# the six Catch cases of eigen_vectors_and_values, cracks.cc:1740-1919
CATCH = [[[2.0, 0.0], [0.0, 3.0]], [[-2.0, 0.0], [0.0, 0.0]], [[5.0, 0.0], [0.0, 0.0]], [[0.0, -2.0], [-2.0, 0.0]],
         [[3.0, 2.0], [2.0, 4.0]], [[0.0, -2.0], [-2.0, 4.0]]]
UNIT2 = [np.array([[1.0, 0.0], [0.0, 0.0]]), np.array([[0.0, 0.0], [0.0, 1.0]]), np.array([[0.0, 0.5], [0.5, 0.0]])]


def _embed(E2):
    E = np.zeros((3, 3))
    E[:2, :2] = E2
    return E


def _random_planar(rng, n):
    """symmetric 2 x 2 tensors of both signs with |E_01| >= 1e-2 |E| (away from the reference's 'close to diagonal' branch)"""
    out = []
    while len(out) < n:
        a, b, s = rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-4, 0)
        E2 = np.array([[a, s], [s, b]])
        if abs(s) >= 1e-2 * np.linalg.norm(E2):
            out.append(E2)
    return out


def _check_planar(E2, derivative_too):
    scale = max(1.0, LAM + 2 * MU) * max(np.abs(E2).max(), 1e-300)
    err, sp_ref, sm_ref = O.decompose_stress_2d(E2, np.zeros((2, 2)), LAM, MU, False)
    assert err == 0
    sp, sm = spectral_split(_embed(E2), LAM, MU)
    assert np.abs(sp[:2, :2] - sp_ref).max() < 1e-13 * scale and np.abs(sm[:2, :2] - sm_ref).max() < 1e-13 * scale
    if not derivative_too:
        return
    Cp, Cm = spectral_tangent(_embed(E2), LAM, MU)
    for H2 in UNIT2:
        err, spL_ref, smL_ref = O.decompose_stress_2d(E2, H2, LAM, MU, True)
        assert err == 0
        H = _embed(H2)
        spL, smL = np.einsum("abcd,cd->ab", Cp, H), np.einsum("abcd,cd->ab", Cm, H)
        # the closed form differentiates through 1 / E_01 and 1 / discriminant (cracks.cc:1982-2006): its own rounding error
        # is amplified by |E| / |E_01| <= 1e2, hence 1e-11 relative to the moduli
        assert np.abs(spL[:2, :2] - spL_ref).max() < 1e-11 * (LAM + 2 * MU)
        assert np.abs(smL[:2, :2] - smL_ref).max() < 1e-11 * (LAM + 2 * MU)


def test_planar_tensors_reproduce_the_2d_closed_form():
    rng = np.random.default_rng(11)
    for E2 in _random_planar(rng, 40):
        _check_planar(E2, True)


@pytest.mark.parametrize("k", range(6))
def test_catch_matrices(k):
    E2 = np.array(CATCH[k])
    # exactly diagonal tensors: the reference's derivative branch divides by E_01 = 0 (tests/test_gpu_split_corners.py),
    # only its stress branch is a reference there
    _check_planar(E2, derivative_too=E2[0, 1] != 0.0)


def _well_separated(rng, n):
    out = []
    while len(out) < n:
        A = rng.uniform(-1, 1, (3, 3))
        E = 0.5 * (A + A.T) + rng.uniform(-1.5, 1.5) * np.eye(3)  # (the shift: definite tensors among them)
        l = np.linalg.eigvalsh(E)
        if np.abs(l).min() >= 1e-2 * np.linalg.norm(E):
            out.append(E)
    return out


def test_tangent_is_the_derivative_of_the_split():
    """Central differences with step h = 1e-5 |E| in every symmetric unit direction.  Away from lambda_i = 0 (asserted:
    min |lambda_i| >= 1e-2 |E| >> h) the split is smooth; with |E| ~ 1 and moduli ~ 3e2 the truncation error is
    O(h^2) |sigma'''| ~ 1e-10 * 3e2 / (1e-2)^2 at worst (third derivatives grow with 1 / gap^2) and the rounding error
    ulp |sigma| / h ~ 1e-16 * 3e2 / 1e-5: both below 1e-6 (lam + 2 mu), the bound used."""
    rng = np.random.default_rng(5)
    tol = 1e-6 * (LAM + 2 * MU)
    signs = set()
    for E in _well_separated(rng, 30):
        signs.add(tuple(np.sign(np.linalg.eigvalsh(E)).astype(int)))
        h = 1e-5 * np.linalg.norm(E)
        Cp, Cm = spectral_tangent(E, LAM, MU)
        for i in range(3):
            for j in range(i, 3):
                H = np.zeros((3, 3))
                H[i, j] = H[j, i] = 1.0 if i == j else 0.5
                sp1, sm1 = spectral_split(E + h * H, LAM, MU)
                sp0, sm0 = spectral_split(E - h * H, LAM, MU)
                assert np.abs((sp1 - sp0) / (2 * h) - np.einsum("abcd,cd->ab", Cp, H)).max() < tol
                assert np.abs((sm1 - sm0) / (2 * h) - np.einsum("abcd,cd->ab", Cm, H)).max() < tol
    assert len(signs) >= 3  # mixed signs of both kinds and at least one definite tensor


def test_tangent_symmetries_and_sum():
    rng = np.random.default_rng(6)
    I = np.eye(3)
    C = LAM * np.einsum("ab,cd->abcd", I, I) + MU * (np.einsum("ac,bd->abcd", I, I) + np.einsum("ad,bc->abcd", I, I))
    for E in _well_separated(rng, 10):
        Cp, Cm = spectral_tangent(E, LAM, MU)
        for T in (Cp, Cm):
            assert np.abs(T - T.transpose(2, 3, 0, 1)).max() < 1e-12 * (LAM + 2 * MU)
            assert np.abs(T - T.transpose(1, 0, 2, 3)).max() < 1e-12 * (LAM + 2 * MU)
        assert np.abs(Cp + Cm - C).max() < 1e-12 * (LAM + 2 * MU)
        sp, sm = spectral_split(E, LAM, MU)
        assert np.abs(sp + sm - (LAM * np.trace(E) * I + 2 * MU * E)).max() < 1e-12 * (LAM + 2 * MU)
        # sigma+ is positively homogeneous of degree one: C+ : E = sigma+
        assert np.abs(np.einsum("abcd,cd->ab", Cp, E) - sp).max() < 1e-12 * (LAM + 2 * MU)


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


@pytest.mark.parametrize("spectrum", [(2.0, 2.0, -1.0), (-2.0, -2.0, 1.0), (0.5, 0.5, 0.25), (1.5, 1.5, 1.5), (-1.5, -1.5, -1.5),
                                      (0.0, 0.0, 0.0)], ids=str)
def test_repeated_eigenspaces_do_not_see_the_basis(spectrum):
    """R diag(l) R^T for random rotations R -- eigh returns another basis of the repeated eigenspace each time -- against
    the closed form of the result: E+ = R diag(l+) R^T, and the tangent rotated as a fourth-order tensor."""
    rng = np.random.default_rng(7)
    D = np.diag(spectrum)
    sp0, sm0 = spectral_split(D, LAM, MU)
    Cp0, Cm0 = spectral_tangent(D, LAM, MU)
    if spectrum == (0.0, 0.0, 0.0):
        Is = 0.5 * (np.einsum("ac,bd->abcd", np.eye(3), np.eye(3)) + np.einsum("ad,bc->abcd", np.eye(3), np.eye(3)))
        assert np.array_equal(Cp0, LAM * np.einsum("ab,cd->abcd", np.eye(3), np.eye(3)) + 2 * MU * Is)  # theta = 1, h(0) = 1
    for _ in range(8):
        R = _rotation(rng)
        E = R @ D @ R.T
        E = 0.5 * (E + E.T)
        sp, sm = spectral_split(E, LAM, MU)
        Cp, Cm = spectral_tangent(E, LAM, MU)
        rot2 = lambda S: R @ S @ R.T
        rot4 = lambda T: np.einsum("ai,bj,ck,dl,ijkl->abcd", R, R, R, R, T)
        tol = 1e-12 * (LAM + 2 * MU) * max(1.0, np.abs(D).max())
        assert np.abs(sp - rot2(sp0)).max() < tol and np.abs(sm - rot2(sm0)).max() < tol
        assert np.abs(Cp - rot4(Cp0)).max() < tol and np.abs(Cm - rot4(Cm0)).max() < tol
        assert np.abs(positive_part(E) - rot2(np.diag(np.maximum(spectrum, 0.0)))).max() < 1e-14 * max(1.0, np.abs(D).max())


# ---- the assembly reference of the GPU tests (tests/split3d_ref.py), checked here without a GPU
def _small_3d_case(split_params):
    import cases
    import split3d_ref  # noqa: F401
    from cracks_amd import mesh as M

    mesh = M.box_mesh(3, (3, 2, 2), lo=0.0, hi=(3.0, 2.0, 2.0))
    rng = np.random.default_rng(2)
    inner = np.setdiff1d(np.arange(mesh.n_nodes), np.concatenate(list(mesh.boundary_nodes.values())))
    mesh.coords[inner] += rng.uniform(-0.12, 0.12, (inner.size, 3))
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=True)
    u = rng.uniform(-1e-2, 1e-2, (mesh.n_nodes, 3))
    vec = lambda uu: lay.pack(uu, rng.uniform(0.3, 0.9, mesh.n_nodes))
    prm = O.make_params(**{"lambda": LAM}, mu=MU, G_c=2.7, alpha_eps=0.5, constant_k=1e-3, pressure=0.05, timestep=1e-3, time=2e-3,
                        old_timestep=1e-3, old_old_timestep=1e-3, outer_solver=1, gamma_penal=10.0, **split_params)
    cu, ch = M.update_constraints(mesh, lay, []), M.hanging_constraints(mesh, lay)
    return cases.Case("ref", mesh, lay, prm, vec(u), vec(0 * u), vec(0 * u), cu, ch)


def test_assembly_reference_reproduces_the_oracle_with_the_split_off():
    import scipy.sparse as sp
    import split3d_ref as R
    from cracks_amd import mesh as M

    c = _small_3d_case(dict(timestep_number=1, decompose_stress_rhs=1.0, decompose_stress_matrix=0.0))
    rowptr, colind = M.dof_sparsity(c.mesh, c.layout)
    r = O.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cu, c.ch, False, rowptr, colind)
    assert r.err == 0
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=(c.layout.n_dofs,) * 2)
    A, res, _ = R.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold)
    assert abs(A - A_ref).max() < 1e-12 * max(1.0, abs(A_ref).max())
    assert np.abs(res - r.residual_pde).max() < 1e-12 * max(1.0, np.abs(r.residual_pde).max())


def test_assembly_reference_with_positive_spectrum_is_the_unsplit_assembly():
    import split3d_ref as R

    c = _small_3d_case(dict(timestep_number=1, decompose_stress_rhs=1.0, decompose_stress_matrix=1.0))
    lay = c.layout
    u, phi = R.nodal(lay, c.sol)
    sol = lay.pack(u + 5e-2 * c.mesh.coords, phi)  # uniform expansion on top: every eigenvalue positive
    A1, r1, E = R.assemble(c.mesh, lay, c.params, sol, c.old, c.oldold, split=True)
    assert np.linalg.eigvalsh(E).min() > 0
    A0, r0, _ = R.assemble(c.mesh, lay, c.params, sol, c.old, c.oldold, split=False)
    assert abs(A1 - A0).max() < 1e-12 * max(1.0, abs(A0).max()) and np.abs(r1 - r0).max() < 1e-12 * max(1.0, np.abs(r0).max())
