"""Tension / compression splits of the stress in 3-D, in plain numpy: the spectral split (below) and the
volumetric-deviatoric split (``voldev_split``, ``voldev_tangent``: ``PFM_SPLIT_VOLDEV``, the law in their docstrings).

Like ``kelly_numpy`` this is both the statement of the law and the reference the device code
(``csrc/pfm_split3.h``, the 3-D SPLIT instantiations of ``k_assemble_general``) is tested against.
The reference application has no 3-D split: its closed form reads the 2 x 2 corner of the strain
(cracks.cc:1683-1690).  ``PFM_SPLIT_SPECTRAL`` is the Miehe-type split through the eigenpairs of E:

    E  = sum_i l_i n_i n_i^T               h(x) = 0 if x < 0 else 1
    E+ = sum_i max(l_i, 0) n_i n_i^T       tr+ = max(tr E, 0)
    sigma+ = lam tr+ I + 2 mu E+           sigma- = lam (tr E - tr+) I + 2 mu (E - E+)

    dE+[H] = sum_i h(l_i) (n_i^T H n_i) n_i n_i^T + sum_{i != j} theta_ij (n_i^T H n_j) n_i n_j^T
    theta_ij = (max(l_i, 0) - max(l_j, 0)) / (l_i - l_j)
    sigma+_LinU = lam h(tr E) tr(H) I + 2 mu dE+[H]
    sigma-_LinU = lam (1 - h(tr E)) tr(H) I + 2 mu (H - dE+[H])

Two conventions:
  * h(0) = 1: zero counts as tension (the reference's ``< 0`` tests, cracks.cc:2068-2101).
  * theta_ij = h(l_i) when l_i == l_j in floating point.  For two eigenvalues of the same sign the
    quotient is exactly 1 or 0, so neither function depends on the basis chosen inside a repeated
    eigenspace.

Tensors may carry leading batch dimensions: E[..., 3, 3].
"""
import numpy as np

VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def _eig(E):
    E = np.asarray(E, dtype=np.float64)
    return np.linalg.eigh(0.5 * (E + np.swapaxes(E, -1, -2)))


def positive_part(E):
    """E+ = sum_i max(l_i, 0) n_i n_i^T."""
    l, n = _eig(E)
    return np.einsum("...i,...ai,...bi->...ab", np.maximum(l, 0.0), n, n)


def spectral_split(E, lam, mu):
    """(sigma+, sigma-) of the strain E; lam, mu scalars or arrays of the batch shape."""
    E = np.asarray(E, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)[..., None, None]
    mu = np.asarray(mu, dtype=np.float64)[..., None, None]
    Ep = positive_part(E)
    tr = np.trace(E, axis1=-2, axis2=-1)[..., None, None]
    trp = np.maximum(tr, 0.0)
    I = np.eye(3)
    return lam * trp * I + 2 * mu * Ep, lam * (tr - trp) * I + 2 * mu * (E - Ep)


def positive_part_tangent(E):
    """dE+/dE as a tensor P[..., a, b, c, d] with both minor symmetries: dE+[H] = P : H."""
    l, n = _eig(E)
    h = np.where(l < 0.0, 0.0, 1.0)
    lp = np.maximum(l, 0.0)
    gap = l[..., :, None] - l[..., None, :]
    same = gap == 0.0
    theta = np.where(same, h[..., :, None], (lp[..., :, None] - lp[..., None, :]) / np.where(same, 1.0, gap))
    T = np.einsum("...ij,...ai,...bj,...ci,...dj->...abcd", theta, n, n, n, n)
    return 0.5 * (T + np.swapaxes(T, -1, -2))


def spectral_tangent(E, lam, mu):
    """(C+, C-): sigma+-_LinU = C+- : H, tensors [..., 3, 3, 3, 3] with major and minor symmetries."""
    E = np.asarray(E, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)[..., None, None, None, None]
    mu = np.asarray(mu, dtype=np.float64)[..., None, None, None, None]
    P = positive_part_tangent(E)
    I = np.eye(3)
    II = np.einsum("ab,cd->abcd", I, I)
    Is = 0.5 * (np.einsum("ac,bd->abcd", I, I) + np.einsum("ad,bc->abcd", I, I))
    htr = np.where(np.trace(E, axis1=-2, axis2=-1) < 0.0, 0.0, 1.0)[..., None, None, None, None]
    return lam * htr * II + 2 * mu * P, lam * (1.0 - htr) * II + 2 * mu * (Is - P)


def voldev_split(E, lam, mu):
    """(sigma+, sigma-) of the volumetric-deviatoric split (``PFM_SPLIT_VOLDEV``; Amor, Marigo, Maurini):

        K = lam + 2 mu / 3          tr+ = max(tr E, 0)          tr- = tr E - tr+
        sigma+ = K tr+ I + 2 mu (E - (tr E / 3) I)              sigma- = K tr- I

    lam, mu scalars or arrays of the batch shape, as in ``spectral_split``."""
    E = np.asarray(E, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)[..., None, None]
    mu = np.asarray(mu, dtype=np.float64)[..., None, None]
    K = lam + 2 * mu / 3
    tr = np.trace(E, axis1=-2, axis2=-1)[..., None, None]
    trp = np.maximum(tr, 0.0)
    I = np.eye(3)
    return K * trp * I + 2 * mu * (E - tr / 3 * I), K * (tr - trp) * I


def voldev_tangent(E, lam, mu):
    """(C+, C-) of the volumetric-deviatoric split, tensors [..., 3, 3, 3, 3] as in ``spectral_tangent``:

        C+ = K h(tr E) I (x) I + 2 mu (I_s - 1/3 I (x) I)       C- = K (1 - h(tr E)) I (x) I

    with h(0) = 1.  Both are isotropic: g C+ + d C- = a I (x) I + 2 b I_s with
    a = lam (g h + d (1 - h)) - (2 mu / 3) (1 - h) (g - d) and b = mu g, which is the form the kernel keeps per q-point."""
    E = np.asarray(E, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)[..., None, None, None, None]
    mu = np.asarray(mu, dtype=np.float64)[..., None, None, None, None]
    K = lam + 2 * mu / 3
    I = np.eye(3)
    II = np.einsum("ab,cd->abcd", I, I)
    Is = 0.5 * (np.einsum("ac,bd->abcd", I, I) + np.einsum("ad,bc->abcd", I, I))
    h = np.where(np.trace(E, axis1=-2, axis2=-1) < 0.0, 0.0, 1.0)[..., None, None, None, None]
    return K * h * II + 2 * mu * (Is - II / 3), K * (1.0 - h) * II


def voigt6(S):
    """The six components 00, 11, 22, 01, 02, 12 of a symmetric tensor."""
    S = np.asarray(S)
    return np.stack([S[..., i, j] for i, j in VOIGT], axis=-1)


def voigt21(C):
    """Packed upper triangle (row by row) of the symmetric 6 x 6 form of a tangent, order of VOIGT.

    Entry (r, k) is stress component r for the unit direction k, a shear direction being
    sym(e_i e_j^T) with DOUBLED shear 1 -- the form the kernel keeps per q-point."""
    C = np.asarray(C)
    return np.stack([C[..., VOIGT[r][0], VOIGT[r][1], VOIGT[k][0], VOIGT[k][1]] for r in range(6) for k in range(r, 6)], axis=-1)
