"""Mesh adaptation without a GPU: the three entry points of include/pfm_newton.h ("mesh adaptation") are declared,
exported and refuse bad arguments; the numpy statement of cracks_amd/adapt.py and its two-level meshes are consistent;
AdaptiveDriver around the oracle reproduces the reference's predictor-corrector run tests/miehe_shear_1.output through
all five mesh changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adapt_cases as AC
import newton_cases as NC
from cracks_amd import adapt as A
from cracks_amd import build, capi
from cracks_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pfm_refine_flags", "pfm_min_cell_diameter", "pfm_state_transfer"]


@pytest.fixture(scope="module")
def lib():
    build.build_native()
    return capi.load()


def test_adaptation_symbols_are_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "pfm_newton.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text))
    for n in NAMES:
        assert n in declared, n
        assert n in capi.EXPORTS, n
        assert hasattr(lib, n), n
    assert "pfm_refine_criteria" in text


def test_refine_criteria_layout_matches_c():
    import subprocess
    import tempfile

    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "pfm_newton.h"
int main(void){
  printf("%zu %zu %zu %zu %zu\n", sizeof(pfm_refine_criteria), offsetof(pfm_refine_criteria, use_box),
         offsetof(pfm_refine_criteria, box_lo), offsetof(pfm_refine_criteria, box_hi), offsetof(pfm_refine_criteria, max_level));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])  # plain C: the header is C-clean
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    R = capi.PfmRefineCriteria
    assert out == [C.sizeof(R), R.use_box.offset, R.box_lo.offset, R.box_hi.offset, R.max_level.offset]


def test_bad_arguments_are_rejected_without_a_gpu(lib):
    crit = capi.PfmRefineCriteria()
    n = C.c_int64(7)
    flags = (C.c_uint8 * 4)()
    assert lib.pfm_refine_flags(None, C.byref(crit), None, None, flags, C.byref(n)) == 1  # PFM_ERR_BAD_ARG
    assert lib.pfm_refine_flags(None, None, None, None, None, None) == 1
    assert n.value == 7
    h = C.c_double(-1.0)
    assert lib.pfm_min_cell_diameter(None, None, C.byref(h)) == 1
    assert lib.pfm_min_cell_diameter(None, None, None) == 1
    assert h.value == -1.0
    ptrs = (C.c_void_p * 3)()
    assert lib.pfm_state_transfer(None, None, None, None, 3, ptrs, ptrs) == 1
    assert lib.pfm_state_transfer(None, None, None, None, 0, None, None) == 1


def test_adapt_module_does_not_use_the_oracle():
    text = open(os.path.join(ROOT, "cracks_amd", "adapt.py")).read()
    assert "oracle" not in text


# ---- the numpy statement ---------------------------------------------------------------------------------------------

def test_flags_numpy_edge_cases():
    m = M.box_mesh(2, 4, 0.0, 4.0)
    phi = np.ones(m.n_nodes)
    phi[0] = 0.5  # corner node of cell 0 only
    phi[12] = 0.8  # equal to the threshold: not flagged
    phi[24] = np.nan
    f, n = A.refine_flags_numpy(m, phi, 0.8)
    assert n == 1 and f[0] == 1
    f, n = A.refine_flags_numpy(m, phi, float("nan"))
    assert n == 0
    f, n = A.refine_flags_numpy(m, phi, float("nan"), box_lo=[-np.inf, 3.5], box_hi=[np.inf, np.inf])
    assert n == 4 and f[12:].all()  # the y >= 3.5 rule with open sides: the top row of cells
    level = np.zeros(m.n_cells, np.uint8)
    level[0] = 1
    f, n = A.refine_flags_numpy(m, phi, 0.8, max_level=1, cell_level=level)
    assert n == 0
    f, n = A.refine_flags_numpy(m, phi, 0.8, cell_owned=np.zeros(m.n_cells, np.uint8))
    assert n == 0
    assert A.min_cell_diameter_numpy(m, np.zeros(m.n_cells, np.uint8)) == np.inf
    assert A.min_cell_diameter_numpy(m) == m.min_cell_diameter()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("blocked", [False, True])
def test_transfer_numpy_reproduces_q1_functions(dim, blocked):
    """A (multi)linear function on the base mesh is in the Q1 space of every refinement: its transfer is its interpolant on
    the new mesh, hanging nodes included; a same-mesh transfer is a bitwise copy."""
    base = M.box_mesh(dim, 4, 0.0, 1.0)
    rng = np.random.default_rng(5)
    m1 = rng.random(base.n_cells) < 0.3
    m2 = m1 | (rng.random(base.n_cells) < 0.3)
    t1 = A.two_level_mesh(base, m1)
    t2 = A.two_level_mesh(base, m2, m1)
    assert A.relation_matches(t1.mesh, t2.mesh, t2.parent_cell, t2.child)
    assert t2.mesh.n_cells == base.n_cells + ((1 << dim) - 1) * int(m2.sum())

    def field(mesh):
        lay = M.DofLayout(mesh.n_nodes, dim, blocked)
        x = mesh.coords
        u = np.stack([1.0 + (d + 1) * x[:, d] + 0.5 * x[:, 0] * x[:, -1] for d in range(dim)], axis=1)
        return lay.pack(u, 2.0 - x[:, 0] * x[:, 1])

    out = A.transfer_numpy(t1.mesh, t2.mesh, blocked, t2.parent_cell, t2.child, [field(t1.mesh)])[0]
    assert np.abs(out - field(t2.mesh)).max() < 1e-14
    # identity relation: a copy, bit for bit (random bits, negative zeros included)
    v = rng.standard_normal(t1.mesh.n_nodes * (dim + 1))
    v[::7] = -0.0
    same = A.transfer_numpy(t1.mesh, t1.mesh, blocked, np.arange(t1.mesh.n_cells), np.full(t1.mesh.n_cells, 255), [v])[0]
    assert same.tobytes() == v.tobytes()
    # broken relations are refused
    bad = t2.parent_cell.copy()
    bad[-1] = (bad[-1] + 1) % t1.mesh.n_cells
    with pytest.raises(ValueError):
        A.transfer_numpy(t1.mesh, t2.mesh, blocked, bad, t2.child, [field(t1.mesh)])
    bad_child = t2.child.copy()
    k = int(np.nonzero(bad_child != 255)[0][0])
    bad_child[k] ^= 1
    assert not A.relation_matches(t1.mesh, t2.mesh, t2.parent_cell, bad_child)
    bad_child[k] = 1 << dim
    assert not A.relation_matches(t1.mesh, t2.mesh, t2.parent_cell, bad_child)


# ---- the reference's adaptive run ------------------------------------------------------------------------------------

def test_miehe_shear_1_adaptive_with_oracle():
    drv = AC.adaptive_miehe_shear_1(NC.OracleAssembler, A.NumpyAdaptor())
    AC.check_adaptive_miehe_shear_1(drv.run())
