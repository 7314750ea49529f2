"""The adaptive run of tests/miehe_shear_1.prm (predictor-corrector refinement, phase-field threshold 0.8, one level above
the 256-cell slit mesh) for cracks_amd.adapt.AdaptiveDriver, and its comparison with the reference's output
(tests/golden/amr_miehe_shear_1.json, made by tests/golden/make_amr_kat.py)."""
import json
import os

import numpy as np
import pytest

import cases
from cracks_amd import mesh as M
from cracks_amd.adapt import AdaptiveDriver
from cracks_amd.newton import ProblemSetup

HERE = os.path.dirname(os.path.abspath(__file__))
PHI_THRESHOLD = 0.8  # "Threshold for phase field refinement" of tests/miehe_shear_1.prm


def amr_golden():
    with open(os.path.join(HERE, "golden", "amr_miehe_shear_1.json")) as f:
        return json.load(f)["blocks"]


def miehe_shear_1_setup_of(mesh) -> ProblemSetup:
    """newton_cases.miehe_shear_1_setup on any refinement of the slit mesh (the parameters are those of the finest level,
    cracks.cc:3839-3854)."""
    params = cases.kat_miehe_shear_1().params
    lay = M.DofLayout(mesh.n_nodes, 2, blocked=False)
    top = mesh.boundary_nodes[3]
    dd = M.miehe_shear_dirichlet_dofs(mesh, lay)

    def initial_bc(time):
        vals = {int(d): 0.0 for d in dd}
        for n in top:  # BoundaryShearTest, cracks.cc:838-858
            vals[int(lay.dof(n, 0))] = -1.0 * time
        return vals

    sol0 = lay.pack(np.zeros((mesh.n_nodes, 2)), np.ones(mesh.n_nodes))
    return ProblemSetup(mesh=mesh, layout=lay, params=params, dirichlet_dofs=dd, initial_bc=initial_bc, solution0=sol0,
                        E_modulus=1.0e3, timestep=1.0e-3, max_no_timesteps=10, newton_tol=1.0e-6, max_newton_steps=100,
                        max_line_search=10, line_search_damping=0.6, compute_load=True)


def adaptive_miehe_shear_1(assembler_of, adaptor, log=None) -> AdaptiveDriver:
    return AdaptiveDriver(M.slit_mesh(3), miehe_shear_1_setup_of, assembler_of, adaptor, PHI_THRESHOLD, log=log)


def check_adaptive_miehe_shear_1(records, show=print):
    """The blocks of time steps 6-10 (ten of them: every step is run on two meshes): cell and DoF counts exact, line-0
    residuals at rel 5e-6, energies at rel 5e-6 and the load at rel 3e-6 for steps 6-9 (the tolerances of
    test_newton_goldens._check_miehe_shear_1), last Newton row < 1e-6.  The energies of step 10, where the crack runs, are
    not compared: any two correct implementations differ there by 1e-5 (a borderline active set)."""
    g = amr_golden()
    assert len(g) == 16 and sum(b["mesh_changed"] for b in g) == 5
    assert len(records) == len(g)
    late = [(r, b) for r, b in zip(records, g) if b["timestep"] >= 6]
    assert len(late) == 10
    for r, b in zip(records, g):
        show(f"step {b['timestep']}: cells {r.n_cells}/{b['cells']} dofs {r.n_dofs}/{b['dofs']} changed {r.mesh_changed}/"
             f"{b['mesh_changed']} residual0 {r.residual0:.6e}/{b['residual0']:.6e} last row {r.newton[-1].residual:.3e} "
             f"bulk {r.bulk_energy:.6g}/{b.get('bulk_energy')} crack {r.crack_energy:.6g}/{b.get('crack_energy')} "
             f"load {r.load}/{b.get('load_x')}")
    for r, b in zip(records, g):
        assert r.timestep == b["timestep"]
        assert (r.n_cells, r.n_dofs, r.mesh_changed) == (b["cells"], b["dofs"], b["mesh_changed"])
    for r, b in late:
        assert r.residual0 == pytest.approx(b["residual0"], rel=5e-6)
        assert r.newton[-1].residual < 1e-6
        if not b["mesh_changed"] and b["timestep"] <= 9:
            assert r.bulk_energy == pytest.approx(b["bulk_energy"], rel=5e-6)
            assert r.crack_energy == pytest.approx(b["crack_energy"], rel=5e-6)
            assert r.load == pytest.approx(b["load_x"], rel=3e-6)
    assert [r.n_flagged for r, b in zip(records, g) if b["mesh_changed"]] == [2, 6, 8, 11, 35]
