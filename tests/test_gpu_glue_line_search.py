"""PfmGlue::line_search of glue/cracks_gpu_assemble.cc through the mock of tests/test_glue_mock.py
(tests/cpp/glue_ls_driver.cpp), on one rank in both forms: line_search_stepwise false (one pfm_line_search_device call) and
true (the host loop of a rank with ghost peers).  Both leave the same P.solution, P.system_total_residual and result, and
these equal the composition of the Python entries; P.system_total_residual is refreshed although the residuals stay on the
device (residual_to_host = false), which closes the stale-vector finding of the INTEGRATION.md line-search recipe."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_search_cases as L
from cracks_amd import build
from gpu_util import TOL, linf_scaled, make_context
from test_glue_mock import GLUE, MOCK, ROOT, _write_problem

SRC = os.path.join(ROOT, "tests", "cpp", "glue_ls_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "glue_ls_driver")


def build_driver(force=False):
    lib = build.build_native()
    deps = [SRC, GLUE, lib, os.path.join(MOCK, "mock_dealii.h"), os.path.join(ROOT, "tests", "cpp", "glue_driver.cpp")]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir = os.path.dirname(lib)
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-I" + MOCK,
                           "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lpfm_hip", "-Wl,-rpath," + libdir, "-o", EXE])
    return EXE


def test_line_search_driver_compiles_against_the_mock_headers():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver(force=True))
    text = open(GLUE).read()
    assert "pfm_line_search_device" in text and "fetch_total_residual" in text and "line_search_stepwise" in text


def _python_searches(c, upd, norm, restore):
    """the three searches of the driver from the Python entries: (references, [(steps, accepted, norms, sol, tot)])"""
    from test_gpu_newton_device import padded

    import torch

    ctx = make_context(c)
    n = c.layout.n_dofs
    out, refs = [], [float("inf"), 0.0, None]
    for k in range(3):
        ctx.state_set_host(c.sol, c.old, c.oldold)
        v = dict(sol=padded(c.sol), upd=padded(upd), pde=padded(np.zeros(n)), tot=padded(np.zeros(n)), saved=padded(np.zeros(n)))
        steps, accepted, norms, trials = L.compose(ctx, v["sol"], v["upd"], v["pde"], v["tot"], v["saved"], refs[k], 4, L.DAMPING, norm, restore)
        torch.cuda.synchronize()
        out.append((steps, accepted, norms, v["sol"].cpu().numpy()[:n], v["tot"].cpu().numpy()[:n]))
        if k == 1:
            assert trials[0] > trials[1] > trials[2]
            refs[2] = 0.5 * (trials[1] + trials[2])  # trials 0 and 1 are rejected, trial 2 is accepted
    ctx.close()
    return refs, out


CASES = ["box3d_333_blocked", "sneddon_2d_hanging", "box3d_322_interleaved"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_glue_line_search_in_both_forms(name, tmp_path):
    exe = build_driver()
    maker, bitwise, norm, restore = L.LOOP_CASES[name]
    c = maker()
    upd = L.newton_update(c)
    d = str(tmp_path)
    to_mock, _ = _write_problem(c, d, seed=7)
    y = np.empty_like(upd)
    y[to_mock] = upd
    y.tofile(os.path.join(d, "upd.bin"))
    refs, want = _python_searches(c, upd, norm, restore)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe, d, str(int(norm == "linf")), str(int(restore == "subtract")), repr(refs[2])], capture_output=True, text=True,
                       timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_ls_driver: OK" in r.stdout, r.stdout + r.stderr
    read = lambda f, k, what: np.fromfile(os.path.join(d, f"ls_f{f}_k{k}_{what}.bin"))
    node, comp = c.layout.node_comp_of_dof()
    for k, (steps, accepted, norms, sol, tot) in enumerate(want):
        assert (steps, accepted) == [(0, True), (4, False), (2, True)][k]
        res = [read(f, k, "res") for f in (0, 1)]
        print(name, k, res[0], res[1], norms)
        for f in (0, 1):  # against the Python composition
            assert (int(res[f][0]), bool(res[f][1])) == (steps, accepted)
            assert np.allclose(res[f][2:5], norms, rtol=1e-12, atol=0.0)
            s = read(f, k, "sol")[to_mock]
            assert np.array_equal(s.view(np.uint64), sol.view(np.uint64))  # the vector statements are bitwise
            assert linf_scaled(read(f, k, "tot")[to_mock], tot) < TOL
            assert max(res[f][5:7]) == res[f][3]
        # the two forms against each other: identical where the assembly is reproducible bit for bit (the boxes; the
        # general family adds the cells at hanging nodes atomically)
        assert np.array_equal(read(0, k, "sol").view(np.uint64), read(1, k, "sol").view(np.uint64))
        if bitwise:
            assert np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64))
            assert np.array_equal(read(0, k, "tot").view(np.uint64), read(1, k, "tot").view(np.uint64))
        else:
            assert np.allclose(res[0], res[1], rtol=1e-12, atol=0.0)
            assert linf_scaled(read(0, k, "tot"), read(1, k, "tot")) < TOL
