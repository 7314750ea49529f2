"""The metric of tests/parity_scale.py, tested on the CPU with the references alone.

1. The references stay inside a tenth of the bar (<= 1e-13 on each of the four checks).
   3-D: the oracle against tests/split3d_ref.py with the unsplit law; the spectral (split3d_ref) and volumetric-deviatoric
   (split_voldev_ref) laws, which the oracle does not have in 3-D, against themselves under a seeded renumbering of cells and
   vertices.  2-D: the oracle against itself under such a renumbering (another summation order in every row).
   Measured (per entry / worst block / per row / worst part; residual_pde and residual_total together):
     sneddon_3d(4) perturbed   1.0e-15 / 5.5e-16 / 3.5e-16 / 5.4e-16      hetero_3d perturbed   1.9e-15 / 1.6e-15 / 4.1e-16 / 4.9e-16
     hetero_3d step 0          4.2e-15 / 4.1e-15 / 5.5e-16 / 1.9e-15
   Largest of the four per group: 3-D oracle against split3d_ref 4.2e-15; 2-D oracle against itself renumbered 6.3e-16; spectral
   law against itself renumbered 1.1e-15; volumetric-deviatoric law 3.2e-16 -- a twentieth of the 1e-13 asked for.
   Left out of the 3-D comparison for run time alone: the (16, 9, 30) balanced boxes (4320 cells through the einsum reference
   take most of a minute each) -- the same element code runs on (9, 5, 11) and (5, 4, 61) in every variant; and the boxes of
   test_gpu_cart.py beyond the cart_box entries of GPU_CASES, which differ from those in size only.
2. The precondition of the per-entry scale, |ref_ij| <= (1 + 1e-12) sqrt(|d_i| |d_j|), on every case of GPU_CASES.
3. Sensitivity.  Each block and each residual part of the oracle's output rounded to float32 in turn: rejected by the new
   checks on every case (a block that float32 holds exactly -- the (u,u) block of a step-0 state is not one, a residual part
   that is exactly zero is -- is no mutation and is passed over).  On the balanced cases one parameter at a time nudged by a
   relative 1e-8 -- lambda, mu (or the per-cell moduli), G_c, alpha_eps, pressure, gamma_penal where the scheme uses it --
   : the nudged oracle run is rejected.  constant_k is left out: kappa = 1e-8 h enters as (1 - kappa) and as kappa next to
   phi^2 ~ 1, so a relative 1e-8 of it is 1e-16 h of any entry at most, far below what a 1e-12 bar can see.
4. ACCEPTED_BY_LINF_SCALED: the mutations of 3. that the project's older check, gpu_util.linf_scaled with max(1, |ref|_inf)
   over the whole matrix or vector, lets through -- the gap this metric closes.  The test asserts the list as it is.
5. The balance condition of tests/balanced_cases.py on every balanced case, and the trace margin of the split state."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import balanced_cases as B
import cases
import oracle_api as O
import parity_scale as PS
import split3d_ref as R
import split_voldev_cases as SC
import split_voldev_ref as V
import test_gpu_cart as TC
from cracks_amd import mesh as M
from gpu_util import TOL, linf_scaled, oracle, reference_matrix, total_matrix

TENTH = 1e-13


# ---- the cases the GPU tests use ----------------------------------------------------------------------------------------
def _kat(f, pert):
    c = f(4) if f is cases.kat_sneddon_3d else f()
    return cases.perturbed(c) if pert else c


GPU_CASES = {}
for _f in cases.ALL_KATS:
    GPU_CASES[_f.__name__[4:] + "/step0"] = functools.partial(_kat, _f, False)  # the seven golden residuals of test_gpu_parity.py
    GPU_CASES[_f.__name__[4:] + "/perturbed"] = functools.partial(_kat, _f, True)
GPU_CASES["smoke/sneddon_3d(6)"] = lambda: cases.perturbed(cases.kat_sneddon_3d(6))
for _dim, _n, _lo, _hi in [TC.BOXES[0], TC.BOXES[1], TC.BOXES[4]]:  # the Sneddon-material boxes of test_gpu_cart.py
    for _mono in (False, True):
        GPU_CASES[f"cart_box/{_n}/{'monolithic' if _mono else 'staggered'}"] = functools.partial(TC.box_case, _dim, _n, _lo, _hi, True, monolithic=_mono)
BALANCED = {"balanced/" + B.case_id(a): functools.partial(B.balanced_case, *a) for a in B.NAMES}
GPU_CASES.update(BALANCED)


class Out:
    """the oracle's outputs of a case and the matrices their scales come from"""

    def __init__(self, c):
        self.c = c
        self.A = reference_matrix(c)
        r2, _, _ = oracle(c, True)
        self.pde, self.tot = r2.residual_pde, r2.residual_total
        self.A_tot = total_matrix(c, self.A)

    def errors(self, A=None, pde=None, tot=None):
        """the four checks (worst of each) of a mutated output against this one"""
        c, e = self.c, {"entry": 0.0, "block": 0.0, "row": 0.0, "part": 0.0}
        if A is not None:
            e["entry"], blocks = PS.matrix_errors(A, self.A, c.layout)
            e["block"] = max(blocks.values())
        for v, ref, mat in ((pde, self.pde, self.A), (tot, self.tot, self.A_tot)):
            if v is not None:
                row, parts = PS.residual_errors(v, ref, mat, c.layout, c.sol)
                e["row"], e["part"] = max(e["row"], row), max(e["part"], max(parts.values()))
        return e

    def old_check(self, A=None, pde=None, tot=None):
        """gpu_util.linf_scaled, as full_parity applied it before"""
        e = 0.0
        if A is not None:
            e = max(e, linf_scaled(A.data, self.A.data))
        if pde is not None:
            e = max(e, linf_scaled(pde, self.pde))
        if tot is not None:
            e = max(e, linf_scaled(tot, self.tot))
        return e


@functools.lru_cache(maxsize=None)
def out(name):
    return Out(GPU_CASES[name]())


def rejected(e):
    return max(e.values()) > TOL


# ---- 1: reference against reference ---------------------------------------------------------------------------------------
def renumbered(c, seed=7):
    """the same case with vertices and cells in a seeded random order -> (case, dof map old -> new)"""
    rng = np.random.default_rng(seed)
    mesh, lay = c.mesh, c.layout
    p = rng.permutation(mesh.n_nodes)
    order = rng.permutation(mesh.n_cells)
    coords = np.empty_like(mesh.coords)
    coords[p] = mesh.coords
    new = M.Mesh(dim=mesh.dim, coords=coords, cells=np.ascontiguousarray(p[mesh.cells][order].astype(np.int32)),
                 boundary_nodes={k: p[v] for k, v in mesh.boundary_nodes.items()}, hn_nodes=p[mesh.hn_nodes].astype(np.int32), hn_ptr=mesh.hn_ptr,
                 hn_parents=p[mesh.hn_parents].astype(np.int32), hn_weights=mesh.hn_weights)
    node, comp = lay.node_comp_of_dof()
    dmap = lay.dof(p[node], comp)

    def vec(v):
        w = np.empty_like(v)
        w[dmap] = v
        return w

    def cs(s):
        return M.ConstraintSet.from_lines(lay.n_dofs, {int(dmap[d]): [(int(dmap[k]), w) for k, w in ent] for d, ent in s.lines().items()})

    cl = None if c.cell_lambda is None else np.ascontiguousarray(c.cell_lambda[order])
    cm = None if c.cell_mu is None else np.ascontiguousarray(c.cell_mu[order])
    return cases.Case(c.name + "/renumbered", new, lay, c.params, vec(c.sol), vec(c.old), vec(c.oldold), cs(c.cu), cs(c.ch), None, cl, cm), dmap


def back(A, dmap):
    A = sp.csr_matrix(A)[dmap][:, dmap].tocsr()
    A.sort_indices()
    return A


def _worst(e):
    return max(e.values())


REFERENCE_3D = ["sneddon_3d/perturbed", "sneddon_3d/step0", "hetero_3d/perturbed", "hetero_3d/step0", "smoke/sneddon_3d(6)"] + \
               [k for k in GPU_CASES if k.startswith("cart_box/") and k.count(",") == 2] + [k for k in BALANCED if k.count("x") == 2 and "16x9x30" not in k]
REFERENCE_2D = [k for k in GPU_CASES if k.split("/")[0] in ("threepoint", "sneddon_2d", "miehe_shear_1", "miehe_shear_2", "miehe_tension")] + \
               ["cart_box/(12, 7)/staggered", "cart_box/(12, 7)/monolithic"] + [k for k in BALANCED if k.count("x") == 1]


@pytest.mark.parametrize("name", REFERENCE_3D)
def test_oracle_and_numpy_reference_agree_in_3d(name):
    o = out(name)
    c = o.c
    args = (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
    A, res, _ = R.assemble(*args, split=False, cu=c.cu, ch=c.ch)
    pde, tot, _ = R.assemble_residuals(*args, split=False, cu=c.cu, ch=c.ch)
    e = o.errors(A, pde, tot)
    e_full = o.errors(None, res, None)
    print(f"reference/reference 3-D {name}: {e} full-assembly residual {e_full['row']:.1e} / {e_full['part']:.1e}")
    assert _worst(e) <= TENTH and _worst(e_full) <= TENTH


@pytest.mark.parametrize("name", REFERENCE_2D)
def test_oracle_agrees_with_itself_renumbered_in_2d(name):
    o = out(name)
    c2, dmap = renumbered(o.c)
    A2 = back(reference_matrix(c2), dmap)
    r2, _, _ = oracle(c2, True)
    e = o.errors(A2, r2.residual_pde[dmap], r2.residual_total[dmap])
    print(f"reference/reference 2-D {name}: {e}")
    assert _worst(e) <= TENTH


@pytest.mark.parametrize("law", ["spectral", "voldev"])
def test_split_laws_agree_with_themselves_renumbered(law):
    """the numpy references of the two 3-D laws: element matrices formed cell by cell, so the renumbering changes the order
    of every row's sum and of the constraint expansion"""
    mod = R if law == "spectral" else V
    c = SC.entry_case("box", True, (1.0, 1.0), True) if law == "voldev" else SC.hanging_case(True, 0)
    c2, dmap = renumbered(c)

    def run(k):
        args = (k.mesh, k.layout, k.params, k.sol, k.old, k.oldold, k.cell_lambda, k.cell_mu)
        A, _, _ = mod.assemble(*args, split=True, cu=k.cu, ch=k.ch)
        pde, tot, _ = mod.assemble_residuals(*args, split=True, cu=k.cu, ch=k.ch)
        return A, pde, tot

    A, pde, tot = run(c)
    A2, pde2, tot2 = run(c2)
    e_entry, blocks = PS.matrix_errors(back(A2, dmap), A, c.layout)
    A_tot = A
    if c.params.outer_solver == 0:
        args = (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
        A_tot, _, _ = mod.assemble(*args, split=True, cu=c.ch, ch=c.ch)
    rows = [PS.residual_errors(pde2[dmap], pde, A, c.layout, c.sol), PS.residual_errors(tot2[dmap], tot, A_tot, c.layout, c.sol)]
    worst = max([e_entry, max(blocks.values())] + [r[0] for r in rows] + [max(r[1].values()) for r in rows])
    print(f"reference/reference {law} {c.name}: entry {e_entry:.1e} blocks {blocks} rows {rows}")
    assert worst <= TENTH


# ---- 2: the precondition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_cauchy_schwarz_precondition(name):
    cs = PS.cauchy_schwarz(out(name).A)
    assert cs <= 1.0 + 1e-12, cs


# ---- 3, 4: sensitivity ------------------------------------------------------------------------------------------------------
def f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def float32_mutations(o):
    """(label, kwargs for Out.errors) of every block and residual part rounded to float32; exact ones are left out"""
    c = o.c
    phi = PS.is_phi(c.layout)
    blk = PS.block_of_entries(c.layout, PS.entry_rows(o.A), o.A.indices)
    for b, label in ((0, "uu"), (2, "phiu"), (3, "phiphi")):
        data = o.A.data.copy()
        data[blk == b] = f32(data[blk == b])
        if not np.array_equal(data, o.A.data):
            yield label, dict(A=sp.csr_matrix((data, o.A.indices, o.A.indptr), shape=o.A.shape))
    for key, ref in (("pde", o.pde), ("tot", o.tot)):
        for part, mask in (("u", ~phi), ("phi", phi)):
            v = ref.copy()
            v[mask] = f32(v[mask])
            if not np.array_equal(v, ref):
                yield f"{key}_{part}", {key: v}


# what gpu_util.linf_scaled (max(1, |ref|_inf) over the whole matrix / vector) accepts of the float32 mutations; every one of
# them is rejected by the new checks.  case -> labels
ACCEPTED_BY_LINF_SCALED = {  # (measured linf_scaled of the mutation; the bar is 1e-12)
    "threepoint/step0": ("phiphi",),  # 2.0e-13
    "threepoint/perturbed": ("phiphi",),  # 2.1e-13
    "miehe_shear_1/step0": ("phiphi",),  # 6.0e-14
    "miehe_shear_1/perturbed": ("phiphi",),  # 1.2e-13
    "miehe_shear_2/step0": ("phiphi",),  # 1.1e-13
    "miehe_shear_2/perturbed": ("phiphi",),  # 1.2e-13
    "miehe_tension/step0": ("phiphi",),  # 4.1e-14
    "miehe_tension/perturbed": ("phiphi",),  # 1.2e-13
    "balanced/9x5x11-blocked-staggered-miehe": ("phiphi",),  # 5.9e-13
}


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_float32_rounding_of_one_block_or_part_is_rejected(name):
    o = out(name)
    accepted = []
    n = 0
    for label, kw in float32_mutations(o):
        e = o.errors(**kw)
        old = o.old_check(**kw)
        n += 1
        if old < TOL:
            accepted.append(label)
        print(f"float32 {name} {label}: new checks {e}  linf_scaled {old:.1e}{'  ACCEPTED before' if old < TOL else ''}")
        assert rejected(e), (name, label, e)
        if label in ("uu", "phiu", "phiphi"):
            assert e["block"] > 1e-9, "float32 is 6e-8 of the block's largest entry at most; the per-block check sees it"
    assert n >= 3, "every case has a matrix"
    assert tuple(accepted) == tuple(ACCEPTED_BY_LINF_SCALED.get(name, ())), (name, accepted)


def nudges(c):
    """(label, case) with one parameter moved by a relative 1e-8"""
    f = 1.0 + 1e-8

    def with_params(**kw):
        prm = O.PfmParams.from_buffer_copy(bytes(c.params))
        for k, v in kw.items():
            setattr(prm, k, v)
        return cases.Case(c.name, c.mesh, c.layout, prm, c.sol, c.old, c.oldold, c.cu, c.ch, None, c.cell_lambda, c.cell_mu)

    if c.cell_lambda is None:
        yield "lambda", with_params(lambda_=c.params.lambda_ * f)
        yield "mu", with_params(mu=c.params.mu * f)
    else:  # per-cell moduli: the parameters' pair is not read
        k = with_params()
        k.cell_lambda = c.cell_lambda * f
        yield "cell_lambda", k
        k = with_params()
        k.cell_mu = c.cell_mu * f
        yield "cell_mu", k
    yield "G_c", with_params(G_c=c.params.G_c * f)
    yield "alpha_eps", with_params(alpha_eps=c.params.alpha_eps * f)
    if c.params.pressure != 0.0:
        yield "pressure", with_params(pressure=c.params.pressure * f)
    if B.present(c, "penalty"):
        yield "gamma_penal", with_params(gamma_penal=c.params.gamma_penal * f)


# the nudges linf_scaled accepts: none on the balanced cases (measured) -- a relative 1e-8 of a parameter moves the largest block
# by about 1e-8 of itself, which one scale for everything sees as well.  What that scale misses is which block moved.
NUDGES_ACCEPTED_BY_LINF_SCALED = {}


@pytest.mark.parametrize("name", list(BALANCED))
def test_a_parameter_nudged_by_1e_8_is_rejected_on_the_balanced_cases(name):
    o = out(name)
    accepted = []
    for label, k in nudges(o.c):
        A = reference_matrix(k)
        r, _, _ = oracle(k, True)
        e = o.errors(A, r.residual_pde, r.residual_total)
        old = o.old_check(A, r.residual_pde, r.residual_total)
        if old < TOL:
            accepted.append(label)
        print(f"nudge {name} {label}: new checks {e}  linf_scaled {old:.1e}{'  ACCEPTED before' if old < TOL else ''}")
        assert rejected(e), (name, label, e)
    assert tuple(accepted) == tuple(NUDGES_ACCEPTED_BY_LINF_SCALED.get(name, ())), (name, accepted)


# ---- 5: the balanced states ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", B.NAMES, ids=[B.case_id(a) for a in B.NAMES])
def test_balance_condition(a):
    c = B.balanced_case(*a)
    m = B.balance_medians(c)
    for fam in B.FAMILIES:
        for where, fams in B.ENTERS.items():
            assert ((where, fam) in m) == (fam in fams and B.present(c, fam))
    print(f"balance {c.name}: " + " ".join(f"{k[0]}/{k[1]}={v:.1e}" for k, v in m.items()))
    assert min(m.values()) >= B.BALANCE, m


def test_the_split_state_has_no_q_point_on_the_edge_of_the_law():
    assert B.trace_margin(B.voldev_case()) >= B.TRACE_MARGIN


# ---- the helper itself ----------------------------------------------------------------------------------------------------------
def test_where_the_scale_is_zero():
    lay = M.DofLayout(2, 1, blocked=True)  # dofs: u0 u1 | phi0 phi1
    A = sp.csr_matrix(np.array([[4.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [2.0, 0.0, 9.0, 3.0], [0.0, 0.0, 3.0, 1.0]]))
    full = sp.csr_matrix((np.ones(16), np.tile(np.arange(4), 4), np.arange(0, 17, 4)), shape=(4, 4))
    ref = sp.csr_matrix((A.toarray().ravel(), full.indices, full.indptr), shape=(4, 4))
    assert PS.matrix_errors(ref, ref, lay)[0] == 0.0
    bad = ref.copy()
    bad.data[6] = 1e-300  # (u1, phi0): s = 0 in the structurally zero block, the smallest difference counts
    assert PS.matrix_errors(bad, ref, lay)[0] == np.inf
    bad = ref.copy()
    bad.data[1] = np.nextafter(1.0, 2.0)  # (u0, u1): d_1 = 0 -- no per-entry scale; the block check sees it
    assert PS.entry_error(bad.data, ref.data, PS.entry_scale(ref)) == (0.0, 7)  # (row and column of u1: seven stored entries)
    assert PS.matrix_errors(bad, ref, lay)[1]["uu"] == pytest.approx(2.0 ** -52 / 4.0)
    bad = ref.copy()
    bad.data[2] = 1e-300  # (u0, phi0): the reference block is all zero
    assert PS.matrix_errors(bad, ref, lay)[1]["uphi"] == np.inf
    sol = np.array([0.0, 0.0, 0.5, 0.5])
    s = PS.residual_scale(ref, lay, sol)
    assert s[1] == 0.0 and s[0] == 2.0  # row u1: only u columns (w = |sol| = 0); row u0: |A_phi0,u0| * 1
    r = np.array([1.0, 0.0, 1.0, 1.0])
    assert PS.residual_errors(r, r, ref, lay, sol)[0] == 0.0
    r2 = r.copy()
    r2[1] = 1e-300
    assert PS.residual_errors(r2, r, ref, lay, sol)[0] == np.inf
    assert PS.block_error(np.zeros(3), np.zeros(3)) == 0.0 and PS.block_error(np.array([np.nan]), np.ones(1)) == np.inf


# ---- entries without a per-entry scale ------------------------------------------------------------------------------------------
def _flat_2d():
    import test_gpu_overlap_phases as OP

    return OP.global_case(2, (12, 7), "flat", True)


DEAD = {"dead_zone_3d": lambda: TC.dead_zone(TC.box_case(3, (6, 5, 4), -10.0, 10.0, True, monolithic=True)),
        "dead_zone_2d": lambda: TC.dead_zone(TC.box_case(2, (12, 7), -10.0, 10.0, False, monolithic=True)),
        "flat_2d": _flat_2d}  # dead zone plus G_c = 0 and no displacement on y > 0: the (phi,phi) diagonal vanishes there too


@pytest.mark.parametrize("name", list(DEAD))
def test_entries_without_a_scale_are_those_next_to_a_vanishing_diagonal(name):
    """The dead zones of tests/test_gpu_cart.py (kappa = 0 and both old phase fields zero in whole cells, so g = 0 there) are
    the states of the GPU suite on which the precondition |ref_ij| <= s_ij fails: the (u,u) diagonal of a displacement dof
    inside the zone is exactly zero, while the coupling (1 - kappa) phi sigma:eps(N_j) N_i of the (phi,u) block, which does
    not carry g, is not.  There s_ij = 0 != ref_ij.  The 'flat' state of tests/test_gpu_overlap_phases.py adds G_c = 0 and zero
    strain on y > 0, where the (phi,phi) diagonal vanishes as well and the pressure term 2 p phi N_i dN_j of (phi,u) does not.
    Asserted: such entries exist, every one of them is a (phi,u) entry whose row or column has a zero diagonal (in the dead
    zones alone: the column), the precondition holds at every other entry, and a second reference (3-D: split3d_ref; 2-D:
    the oracle renumbered) differs from the oracle at some of them -- equality is not something the references give each
    other -- while staying within a tenth of the bar at the block's scale.
    Measured: 3-D 774 such entries (the references differ at 662 of them, by at most 3.2e-16 of |phiu|_inf), 2-D 346 (9, 6.6e-17),
    flat 544 (19, 7.2e-17)."""
    c = DEAD[name]()
    A = reference_matrix(c)
    s = PS.entry_scale(A)
    rows = PS.entry_rows(A)
    blk = PS.block_of_entries(c.layout, rows, A.indices)
    without = (s == 0.0) & (blk != 1)  # what parity_scale.entry_error leaves to the per-block check
    no_scale = without & (A.data != 0.0)
    assert no_scale.sum() > 0
    d = A.diagonal()
    assert (blk[no_scale] == 2).all() and ((d[A.indices[no_scale]] == 0.0) | (d[rows[no_scale]] == 0.0)).all()
    if name.startswith("dead_zone"):
        assert (d[A.indices[no_scale]] == 0.0).all()
    cs = PS.ratio(np.abs(A.data[~without]), s[~without])
    if name.startswith("dead_zone"):
        assert cs <= 1.0 + 1e-12
    else:  # flat: with G_c = 0 the (phi,phi) diagonal next to the zero-strain region is tiny, not zero, and the pressure term
        # of (phi,u) exceeds s_ij there (measured 645 s_ij).  Where s_ij > 0 the per-entry check stays on: it is then
        # stricter than the block's scale, never looser
        assert 1.0 < cs < 1e4
    if c.mesh.dim == 3:
        A2, _, _ = R.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu, split=False, cu=c.cu, ch=c.ch)
        A2 = PS.on_pattern(A2, A)
    else:
        c2, dmap = renumbered(c)
        A2 = back(reference_matrix(c2), dmap)
    diff = np.abs(A2.data - A.data)[no_scale]
    worst = diff.max() / np.abs(A.data[blk == 2]).max()
    print(f"no per-entry scale {name}: {int(no_scale.sum())} entries, references differ at {int((diff != 0).sum())}, at most {worst:.1e} of |phiu|_inf")
    assert (diff != 0.0).any() and worst <= TENTH
    e_entry, n = PS.entry_error(A2.data, A.data, s, blk == 1)
    assert n == without.sum() and e_entry <= TENTH
