"""The float64 numpy statements of the COD bucket profile and the point evaluation (cracks_amd/statistics.py:
cod_buckets_numpy, point_eval_numpy -- what the device entries pfm_cod_buckets / pfm_point_eval are compared against in
tests/test_gpu_statistics2.py), validated on their own: analytic bucket volumes, the reference's printed PStress column
through the oracle-driven Newton harness, an affine field, and the cell rule."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import newton_cases as NC
import statistics_cases as SC
from cracks_amd import build, capi
from cracks_amd import mesh as M
from cracks_amd import statistics as S
from cracks_amd.newton import ActiveSetDriver

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "point_stress.json")


def point_stress_golden():
    with open(GOLDEN) as f:
        return [float(s) for s in json.load(f)["threepoint_1.mpirun=2"]["pstress"]]


def test_bucket_volumes_are_analytic():
    """x in [-1.5, 1.5] in 75 buckets centred at -1.5 + 0.04 i: bucket 0 is half a slice, the half slice at +1.5 has index
    75 and is dropped; the mesh is 3 high."""
    mesh = SC.box2d()
    info = {}
    values, volume = S.cod_buckets_numpy(mesh, SC.smooth_nodal(mesh), info=info)
    assert info["tie_margin"] > 3e-2
    want = np.full(75, 0.04 * 3.0)
    want[0] = 0.02 * 3.0
    # a bucket adds 16 columns x 800 rows of points: at most 12800 roundings of 1.1e-16 relative
    bound = 12800 * 1.2e-16
    assert np.max(np.abs(volume - want)) < bound * 0.12
    assert volume.sum() == pytest.approx(9.0 - 3.0 * 0.02, rel=bound) and np.abs(values).max() > 1e-6
    # the volumes do not depend on the state, the values do
    v2, vol2 = S.cod_buckets_numpy(mesh, SC.smooth_nodal(mesh, seed=8))
    assert np.array_equal(vol2, volume) and not np.array_equal(v2, values)
    # another summation order of the same statement
    v3, vol3 = S.cod_buckets_numpy(mesh, SC.smooth_nodal(mesh), cells_per_chunk=7)
    assert np.max(np.abs(v3 - values)) <= 2e-15 * np.abs(values).max() and np.max(np.abs(vol3 - volume)) <= 2e-15 * volume.max()
    # an owned mask: the two parts add up
    mask = np.arange(mesh.n_cells) % 3 != 1
    a, b = (S.cod_buckets_numpy(mesh, SC.smooth_nodal(mesh), cell_owned=m) for m in (mask, ~mask))
    assert np.max(np.abs(a[0] + b[0] - values)) <= 2e-15 * np.abs(values).max() and np.max(np.abs(a[1] + b[1] - volume)) <= 2e-15 * volume.max()


def test_buckets_of_a_tcv_integrand():
    """All buckets together on a range that holds every point: the midpoint sum of int u . grad(phi), which converges to the
    Gauss value of tests/postproc_ref.py with n_sub^-2."""
    import postproc_ref as R

    mesh = SC.box3d_warped()
    nodal = SC.smooth_nodal(mesh)
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=True)
    sol = lay.pack(nodal[:, :3], nodal[:, 3])
    want = R.tcv(mesh, lay, sol)
    got = [S.cod_buckets_numpy(mesh, nodal, 5, -2.0, 2.0, n)[0].sum() for n in (4, 8)]
    assert abs(got[1] - want) < 0.3 * abs(got[0] - want) and abs(got[1] - want) < 2e-2 * abs(want)
    vol = S.cod_buckets_numpy(mesh, nodal, 5, -2.0, 2.0, 4)[1].sum()
    x = mesh.coords[mesh.cells]
    assert vol == pytest.approx(27.0, rel=2e-2)  # the warp moves the boundary a little
    assert x.shape == (120, 8, 3)


def test_cod_array_columns():
    cols = S.cod_array_from_sums(np.arange(75.0))
    assert cols.shape == (75, 3) and cols[0, 0] == -1.5 and cols[1, 0] == -1.5 + 1 * 3.0 / 75
    width = (-1.5 + 1 * 3.0 / 75) - (-1.5 + 0 * 3.0 / 75)
    assert np.array_equal(cols[:, 1], np.arange(75.0) / width / 2.0)
    assert cols[0, 2] == 0.0 and cols[12, 2] == 0.0 and cols[13, 2] > 0.0  # |x| >= 1 up to bucket 12 (x = -1.02)
    assert cols[:, 2].max() == pytest.approx(1.92e-3, rel=3e-4)
    assert S.cod_array_error(cols) == pytest.approx(np.sqrt(np.sum((cols[:, 1] - cols[:, 2]) ** 2)))
    assert np.array_equal(np.floor(S.value_to_bucket([-1.5, -1.481, -1.479, 1.479, 1.481])), [0, 0, 1, 74, 75])


def test_fixture_regenerates_from_its_script():
    """make_point_stress.py keeps the printed strings: every number parses, the file is its own canonical dump."""
    with open(GOLDEN) as f:
        text = f.read()
    data = json.loads(text)
    assert text == json.dumps(data, indent=1, sort_keys=True) + "\n"
    rec = data["threepoint_1.mpirun=2"]
    assert rec["pstress"][:3] == ["0.000508479", "0.00100935", "0.00149059"] and len(rec["pstress"]) == 9
    assert rec["point"] == ["0.0", "2.0"] and all(float(s) > 0 for s in rec["pstress"])


def _nodal(setup, sol):
    n = np.arange(setup.mesh.n_nodes)
    return np.stack([sol[setup.layout.dof(n, c)] for c in range(setup.mesh.dim + 1)], axis=1)


def test_threepoint_pstress_with_oracle():
    """The reference's PStress column (cracks.cc:3285-3320) from the oracle-driven Newton run.  With the Q1 gradients the
    first three steps deviate from the printed six digits by 6e-8, 4e-7 and 1.2e-6 (relative)."""
    setup = NC.threepoint_setup()
    got, cells = [], []

    def hook(d, rec):
        cell, _, grads = S.point_eval_numpy(setup.mesh, _nodal(setup, d.solution), [(0.0, 2.0)])
        got.append(S.point_stress_from_eval(cell, grads))
        cells.append(int(cell[0]))
        # the two cells that meet at (0, 2) give the same value: the lowest-number rule is harmless there
        for c in np.nonzero(np.any(setup.mesh.cells == top, axis=1))[0]:
            only = np.zeros(setup.mesh.n_cells, np.uint8)
            only[c] = 1
            c2, _, g2 = S.point_eval_numpy(setup.mesh, _nodal(setup, d.solution), [(0.0, 2.0)], only)
            assert int(c2[0]) == c and S.point_stress_from_eval(c2, g2) == pytest.approx(got[-1], rel=1e-9)

    x = setup.mesh.coords
    top = int(np.nonzero((np.abs(x[:, 0]) < 1e-10) & (np.abs(x[:, 1] - 2.0) < 1e-10))[0][0])
    incident = np.nonzero(np.any(setup.mesh.cells == top, axis=1))[0]
    assert incident.tolist() == [9, 171]
    ActiveSetDriver(setup, NC.OracleAssembler(setup.mesh, setup.layout)).run(n_steps=3, step_hook=hook)
    want = point_stress_golden()[:3]
    print("threepoint PStress rel dev", [abs(a / b - 1) for a, b in zip(got, want)])
    assert cells == [9, 9, 9]
    assert got == pytest.approx(want, rel=5e-6)


def _affine(mesh, seed=5):
    rng = np.random.default_rng(seed)
    dim = mesh.dim
    A, b = rng.uniform(-1.0, 1.0, (dim + 1, dim)), rng.uniform(-1.0, 1.0, dim + 1)  # rows: u_0 .. u_{dim-1}, phi
    return A, b, mesh.coords @ A.T + b


@pytest.mark.parametrize("name", ["threepoint", "box3d_warped"])
def test_point_eval_of_an_affine_field(name):
    mesh = {"threepoint": SC.threepoint, "box3d_warped": SC.box3d_warped}[name]()
    dim = mesh.dim
    A, b, nodal = _affine(mesh)
    pts = SC.eval_points(mesh)
    cell, values, grads = S.point_eval_numpy(mesh, nodal, pts)
    inside = cell >= 0
    assert inside[:64].all() and inside.sum() == pts.shape[0] - 4 and not inside[-4:].any()
    assert np.max(np.abs(values[inside] - (pts[inside] @ A.T + b))) < 1e-13
    assert np.max(np.abs(grads[inside] - A[None])) < 1e-13
    assert not values[~inside].any() and not grads[~inside].any()
    # a random interior point lies in the cell it was drawn from
    rng = np.random.default_rng(3)
    assert np.array_equal(cell[:64], rng.integers(0, mesh.n_cells, 64))
    # a shared vertex: the lowest-numbered incident cell, also under a mask that removes it
    counts = np.bincount(mesh.cells.ravel(), minlength=mesh.n_nodes)
    node = int(np.argmax(counts))
    incident = np.nonzero(np.any(mesh.cells == node, axis=1))[0]
    assert incident.size >= (4 if dim == 2 else 8)
    c, v, _ = S.point_eval_numpy(mesh, nodal, mesh.coords[node][None, :])
    assert int(c[0]) == incident[0] and np.max(np.abs(v[0] - nodal[node])) < 1e-13
    mask = np.ones(mesh.n_cells, np.uint8)
    mask[incident[0]] = 0
    assert int(S.point_eval_numpy(mesh, nodal, mesh.coords[node][None, :], mask)[0][0]) == incident[1]
    # no point at all
    c, v, g = S.point_eval_numpy(mesh, nodal, np.zeros((0, dim)))
    assert c.shape == (0,) and v.shape == (0, dim + 1) and g.shape == (0, dim + 1, dim)


def test_point_statistics_without_a_cell():
    class Nowhere:
        dim = 2

        def point_eval(self, points, cell_owned=None):
            return np.array([-1], np.int32), np.zeros((1, 3)), np.zeros((1, 3, 2))

    assert S.point_stress(Nowhere()) == 0.0 and S.point_value(Nowhere(), (0.0, 2.0), 1) == -1e100


def test_abi_rejects_bad_arguments_without_a_gpu():
    build.build_native()
    lib = capi.load()
    out = (C.c_double * 75)()
    assert lib.pfm_cod_buckets(None, None, 75, -1.5, 1.5, 100, out, out) == 1  # PFM_ERR_BAD_ARG
    cell = (C.c_int32 * 1)()
    pts = (C.c_double * 2)()
    assert lib.pfm_point_eval(None, None, 1, pts, cell, None, None) == 1
    assert {"pfm_cod_buckets", "pfm_point_eval"} <= set(capi.EXPORTS)
