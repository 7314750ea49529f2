"""PfmGlue::active_set_update of glue/cracks_gpu_assemble.cc through the mock of tests/test_glue_mock.py
(tests/cpp/glue_as_driver.cpp) on one rank: residual assembly with the residuals left on the device, then two updates, the
second from what the first left.  P.solution, the flag bytes, the cycle counter and the counts equal those of the library
call (pfm_active_set_exchange without peers) made from the Python entries on the same state."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_search_cases as L
from cracks_amd import build
from gpu_util import make_context
from test_glue_mock import GLUE, MOCK, ROOT, _write_problem

SRC = os.path.join(ROOT, "tests", "cpp", "glue_as_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "glue_as_driver")
C_CONST = 10.0


def build_driver(force=False):
    lib = build.build_native()
    deps = [SRC, GLUE, lib, os.path.join(MOCK, "mock_dealii.h"), os.path.join(ROOT, "tests", "cpp", "glue_driver.cpp")]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir = os.path.dirname(lib)
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-I" + MOCK,
                           "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lpfm_hip", "-Wl,-rpath," + libdir, "-o", EXE])
    return EXE


def test_active_set_driver_compiles_against_the_mock_headers():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver(force=True))
    text = open(GLUE).read()
    assert "pfm_active_set_exchange" in text and "active_set_update" in text and "reset_cycle_counter" in text


def _python_updates(c):
    """the two updates from the Python entries: [(counts, solution, flags, cycle counter)]"""
    from test_gpu_newton_device import dev, padded

    import torch

    ctx = make_context(c)
    n, nn = c.layout.n_dofs, c.mesh.n_nodes
    ctx.state_set_host(c.sol, c.old, c.oldold)
    sol, old, pde, tot = padded(c.sol), padded(c.old), padded(np.zeros(n)), padded(np.zeros(n))
    ctx.assemble_device(True, [], pde.data_ptr(), tot.data_ptr())
    mass, cyc = padded(np.zeros(nn)), dev(np.zeros(nn, np.int32))
    ctx.diag_mass_device(mass.data_ptr())
    out = []
    for _ in range(2):
        counts = ctx.active_set_exchange(0, None, tot.data_ptr(), mass.data_ptr(), C_CONST, sol.data_ptr(), old.data_ptr(), cyc.data_ptr())
        torch.cuda.synchronize()
        out.append((counts, sol.cpu().numpy()[:n].copy(), ctx.get_constraints(), cyc.cpu().numpy().copy()))
    ctx.close()
    return out


CASES = ["box3d_322_interleaved", "sneddon_2d_hanging", "hang3d"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_glue_active_set_update_equals_the_library_call(name, tmp_path):
    exe = build_driver()
    c = L.LOOP_CASES[name][0]()
    lay, dim, nn = c.layout, c.mesh.dim, c.mesh.n_nodes
    d = str(tmp_path)
    to_mock, _ = _write_problem(c, d, seed=7)
    want = _python_updates(c)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe, d, repr(C_CONST)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_as_driver: OK" in r.stdout, r.stdout + r.stderr
    rank_of_node = to_mock[lay.dof(np.arange(nn), dim)]  # the mock's phase-field dof of a node ...
    rank_of_node = rank_of_node - dim * nn if lay.blocked else (rank_of_node - dim) // (dim + 1)  # ... to its vertex rank
    hanging = c.ch.flag.astype(bool)
    assert want[0][0][0] > 0 and want[0][0][2] == 1
    for k, (counts, sol, flags, cyc) in enumerate(want):
        read = lambda what, dt: np.fromfile(os.path.join(d, f"as_k{k}_{what}.bin"), dt)
        assert tuple(read("counts", np.int64)) == counts
        assert np.array_equal(read("flags", np.uint8)[rank_of_node], flags)
        assert np.array_equal(read("cyc", np.int32)[rank_of_node], cyc)
        s = read("sol", np.float64)[to_mock]
        assert np.array_equal(s[~hanging].view(np.uint64), sol[~hanging].view(np.uint64))
        # a hanging value: the mock lists the parents in another order; the weights are powers of two, so the products are
        # exact and the sum of at most 4 terms of magnitude <= 1 differs by at most 4 * 2^-52
        assert np.abs(sol).max() <= 1.0 + 1e-12
        assert np.abs(s - sol)[hanging].max(initial=0.0) <= 4 * 2.0 ** -52
    assert want[1][3].any()  # the second update moved cycle counters
