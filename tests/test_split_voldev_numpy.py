"""cracks_amd/split3d.py: voldev_split / voldev_tangent -- the volumetric-deviatoric stress split (PFM_SPLIT_VOLDEV) in numpy --
checked on its own:

* sigma+ + sigma- is the unsplit stress, C+ : E = sigma+;
* away from tr E = 0 the tangents are the derivatives of the stresses (central differences);
* tr E >= 0 gives sigma- = 0 and C- = 0, E = -a I gives sigma+ = 0, and at tr E exactly 0 h = 1;
* the law is invariant under rotation of E.
"""
import numpy as np

from cracks_amd.split3d import voldev_split, voldev_tangent

LAM, MU = 121.15, 80.77
MOD = LAM + 2 * MU
I3 = np.eye(3)
II = np.einsum("ab,cd->abcd", I3, I3)
IS = 0.5 * (np.einsum("ac,bd->abcd", I3, I3) + np.einsum("ad,bc->abcd", I3, I3))


def _tensors(rng, n, margin=0.0):
    """symmetric tensors of magnitude 1e-8 ... 1e4 with traces of both signs, |tr E| >= margin |E|_F"""
    out = []
    while len(out) < n:
        A = rng.uniform(-1, 1, (3, 3))
        E = (0.5 * (A + A.T) + rng.uniform(-1, 1) * I3) * 10.0 ** rng.uniform(-8, 4)
        if abs(np.trace(E)) >= margin * np.linalg.norm(E):
            out.append(E)
    E = np.array(out)
    tr = np.trace(E, axis1=-2, axis2=-1)
    assert (tr > 0).sum() >= n // 4 and (tr < 0).sum() >= n // 4
    return E


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def test_the_parts_add_up_to_the_unsplit_stress_and_the_tangent_reproduces_sigma_plus():
    """Rounding only: 1e-14 relative to (lambda + 2 mu) |E| (a dozen operations on numbers of that size)."""
    rng = np.random.default_rng(1)
    E = _tensors(rng, 200)
    lam, mu = LAM * rng.uniform(0.5, 2.0, 200), MU * rng.uniform(0.5, 2.0, 200)  # arrays of the batch shape
    sp, sm = voldev_split(E, lam, mu)
    Cp, Cm = voldev_tangent(E, lam, mu)
    tr = np.trace(E, axis1=-2, axis2=-1)
    unsplit = lam[:, None, None] * tr[:, None, None] * I3 + 2 * mu[:, None, None] * E
    scale = (lam + 2 * mu) * np.abs(E).max(axis=(-2, -1))
    assert (np.abs(sp + sm - unsplit).max(axis=(-2, -1)) <= 1e-14 * scale).all()
    assert (np.abs(np.einsum("nabcd,ncd->nab", Cp, E) - sp).max(axis=(-2, -1)) <= 1e-14 * scale).all()
    # C+ + C- is the unsplit tangent, and both have the major and minor symmetries
    full = lam[:, None, None, None, None] * II + 2 * mu[:, None, None, None, None] * IS
    assert np.abs(Cp + Cm - full).max() <= 1e-13 * MOD
    for C in (Cp, Cm):
        assert np.array_equal(C, C.transpose(0, 2, 1, 3, 4)) and np.array_equal(C, C.transpose(0, 1, 2, 4, 3))
        assert np.abs(C - C.transpose(0, 3, 4, 1, 2)).max() == 0.0
    # scalars work as the arrays do
    s0, _ = voldev_split(E[0], lam[0], mu[0])
    assert np.array_equal(s0, sp[0])


def test_tangents_are_the_derivatives_of_the_stresses():
    """Central differences with step s = 1e-6 |E| in the six symmetric unit directions, on tensors with |tr E| >= 1e-2 |E|_F
    (asserted by construction: the step cannot cross tr E = 0).  The law is piecewise LINEAR, so the difference quotient
    has no truncation error; its rounding error is ulp |sigma| / s ~ 1e-16 (lam + 2 mu) |E| / (1e-6 |E|): the bound is
    1e-8 (lam + 2 mu)."""
    rng = np.random.default_rng(2)
    dirs = [0.5 * (np.outer(I3[i], I3[j]) + np.outer(I3[j], I3[i])) for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    for E in _tensors(rng, 60, margin=1e-2):
        Cp, Cm = voldev_tangent(E, LAM, MU)
        s = 1e-6 * np.linalg.norm(E)
        for H in dirs:
            sp1, sm1 = voldev_split(E + s * H, LAM, MU)
            sp0, sm0 = voldev_split(E - s * H, LAM, MU)
            assert np.abs((sp1 - sp0) / (2 * s) - np.einsum("abcd,cd->ab", Cp, H)).max() < 1e-8 * MOD
            assert np.abs((sm1 - sm0) / (2 * s) - np.einsum("abcd,cd->ab", Cm, H)).max() < 1e-8 * MOD


def test_one_sided_states_and_the_convention_at_zero_trace():
    rng = np.random.default_rng(3)
    E = _tensors(rng, 100)
    tr = np.trace(E, axis1=-2, axis2=-1)
    sp, sm = voldev_split(E, LAM, MU)
    Cp, Cm = voldev_tangent(E, LAM, MU)
    pos = tr >= 0
    assert pos.any() and (sm[pos] == 0.0).all() and (Cm[pos] == 0.0).all()  # exactly: K * 0 and K * (1 - 1)
    assert (np.abs(sm[~pos] - (LAM + 2 * MU / 3) * tr[~pos, None, None] * I3) <= 1e-15 * MOD * np.abs(tr[~pos, None, None])).all()
    # pure compression E = -a I: sigma+ = 0 (the deviator of a multiple of I vanishes up to the rounding of tr / 3)
    for a in (1e-8, 3e-3, 1.0, 7e3):
        sp, sm = voldev_split(-a * I3, LAM, MU)
        assert np.abs(sp).max() <= 1e-15 * MOD * a
        assert np.abs(sm + (3 * LAM + 2 * MU) * a * I3).max() <= 1e-14 * MOD * a
    # tr E exactly 0: h = 1, zero counts as tension (exact binary fractions: the trace is computed without rounding)
    for E0 in (np.zeros((3, 3)), np.diag([0.5, -0.25, -0.25]), np.array([[0.0, 2.0 ** -8, 0.0], [2.0 ** -8, 0.0, 0.0], [0.0, 0.0, 0.0]])):
        assert np.trace(E0) == 0.0
        sp, sm = voldev_split(E0, LAM, MU)
        Cp, Cm = voldev_tangent(E0, LAM, MU)
        assert (sm == 0.0).all() and (Cm == 0.0).all()
        assert np.abs(sp - 2 * MU * E0).max() <= 1e-15 * MOD * np.abs(E0).max()
        assert np.abs(Cp - (LAM * II + 2 * MU * IS)).max() <= 1e-13 * MOD  # the full, unsplit tangent
    # no NaN for finite input, the extremes of the double range included
    for s in (1e-300, 1e300):
        for sign in (1.0, -1.0):
            out = voldev_split(sign * s * np.diag([1.0, 0.5, 0.25]), LAM, MU) + voldev_tangent(sign * s * I3, LAM, MU)
            assert all(np.isfinite(x).all() for x in out)


def test_invariance_under_rotation():
    """sigma+-(Q E Q^T) = Q sigma+-(E) Q^T and C+-(Q E Q^T) = C+-(E) (isotropic tensors), |tr E| >= 1e-2 |E|_F so that
    the rounding of the rotated trace cannot change its sign.  Bound: rounding of the two rotations, 1e-13 (lam + 2 mu) |E|."""
    rng = np.random.default_rng(4)
    for E in _tensors(rng, 60, margin=1e-2):
        Q = _rotation(rng)
        Er = Q @ E @ Q.T
        Er = 0.5 * (Er + Er.T)
        sp, sm = voldev_split(E, LAM, MU)
        spr, smr = voldev_split(Er, LAM, MU)
        scale = MOD * np.abs(E).max()
        assert np.abs(spr - Q @ sp @ Q.T).max() < 1e-13 * scale and np.abs(smr - Q @ sm @ Q.T).max() < 1e-13 * scale
        Cp, Cm = voldev_tangent(E, LAM, MU)
        Cpr, Cmr = voldev_tangent(Er, LAM, MU)
        assert np.array_equal(Cpr, Cp) and np.array_equal(Cmr, Cm)
        rot = lambda C: np.einsum("ai,bj,ck,dl,ijkl->abcd", Q, Q, Q, Q, C)
        assert np.abs(rot(Cp) - Cp).max() < 1e-12 * MOD and np.abs(rot(Cm) - Cm).max() < 1e-12 * MOD
