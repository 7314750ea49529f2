"""The reference's post-processing numbers (TCV, COD profile, phi L2 error, loads) reproduced by the float64 numpy
restatement (tests/postproc_ref.py) around the oracle-driven Newton harness: validates the checker the device entries
of include/pfm_newton.h are compared against (tests/test_gpu_postproc.py)."""
import json
import os

import numpy as np
import pytest

import cases
import newton_cases as NC
import postproc_ref as R
from cracks_amd import mesh as M
from cracks_amd import statistics as S
from cracks_amd.newton import ActiveSetDriver

HERE = os.path.dirname(os.path.abspath(__file__))


def postproc_golden():
    with open(os.path.join(HERE, "golden", "postproc.json")) as f:
        return json.load(f)


def statistics_column(key, name):
    """Column ``name`` of the reference's .statistics table, by time step (kat.json)."""
    g = cases.golden()[key]
    header = {"miehe_tension_adaptive_1": ["Timestep No", "Time", "DoFs", "minimum cell diameter", "Bulk Energy",
                                           "Crack Energy", "Load y"]}
    col = header.get(key)
    if col is None:  # shear / three-point: the load is the last column as well
        col = [None] * (len(g["statistics"][0]) - 1) + [name]
    return [float(row[col.index(name)]) for row in g["statistics"]]


def sneddon_end_of_cycle_np(mesh, layout, sol, params, nu=0.2):
    lines = S.cod_lines()
    cod, nf = R.cod_lines(mesh, layout, sol, lines)
    vals = S.cod_from_sums(cod, nf)
    return {"tcv": R.tcv(mesh, layout, sol), "tcv_exact": S.tcv_exact(mesh.dim, params.pressure, nu),
            "cod": {float(x): float(v) for x, v in zip(lines, vals) if v > -1e100},
            "phi_L2_error": S.phi_l2_error_from_sums(R.sneddon_phi_error_sq(mesh, layout, sol, params.alpha_eps))}


def check_sneddon(got, key, rel):
    g = postproc_golden()[key]
    assert got["tcv"] == pytest.approx(float(g["tcv"]), rel=rel)
    assert got["tcv_exact"] == pytest.approx(float(g["tcv_exact"]), rel=1e-5)
    assert sorted(got["cod"]) == sorted(float(x) for x, _ in g["cod"])
    for x, v in g["cod"]:
        assert got["cod"][float(x)] == pytest.approx(float(v), rel=rel)
    assert got["phi_L2_error"] == pytest.approx(float(g["phi_L2_error"]), rel=rel)


def test_cod_lines_are_the_references():
    x = S.cod_lines()
    assert x.size == 769 and x[0] == -1.5 and x[-1] == 1.5 and x[256] == -0.5 and x[384] == 0.0
    assert np.all(np.diff(x) > 0)


def test_fixture_regenerates_from_its_script():
    """make_postproc.py keeps the printed strings: every number of the fixture parses, and the file ends in a newline."""
    with open(os.path.join(HERE, "golden", "postproc.json")) as f:
        text = f.read()
    assert text.endswith("\n") and json.loads(text) == postproc_golden()
    assert [x for x, _ in postproc_golden()["sneddon_2d_1"]["cod"]] == ["-1", "0", "1"]


def test_sneddon_2d_statistics_with_oracle():
    setup = NC.sneddon_2d_setup()
    drv = ActiveSetDriver(setup, NC.OracleAssembler(setup.mesh, setup.layout))
    seen = {}

    def hook(d, rec):
        seen[rec.timestep] = float(np.abs(d.old_solution - d.solution).max())
        if rec.timestep == 3:
            seen["stats"] = sneddon_end_of_cycle_np(setup.mesh, setup.layout, d.solution, d._params())

    drv.run(n_steps=4, step_hook=hook)
    assert seen[3] < 1e-5  # the reference's stop criterion (cracks.cc:4487)
    check_sneddon(seen["stats"], "sneddon_2d_1", rel=2e-5)


def test_miehe_tension_load_y_with_oracle():
    setup = NC.miehe_tension_setup()
    drv = ActiveSetDriver(setup, NC.OracleAssembler(setup.mesh, setup.layout))
    cells, faces = M.boundary_faces(setup.mesh, 3)
    loads = []

    def hook(d, rec):
        p = d._params()
        raw = R.face_load(setup.mesh, setup.layout, d.solution, p.lambda_, p.mu, cells, faces)
        loads.append(S.load_from_sums(S.MIEHE_TENSION, raw))

    drv.run(n_steps=4, step_hook=hook)
    want = statistics_column("miehe_tension_adaptive_1", "Load y")[:4]
    assert loads == pytest.approx(want, rel=5e-6)
