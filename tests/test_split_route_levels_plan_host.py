"""PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS / _ALL_LEVELS (13, 15) in the plan of a cartesian assembly
(cracks_amd/csrc/pfm_cart_plan.h: CartPlan::voldev_jac on a level lattice; pfm_set_split_route) as a stand-alone host program
under AddressSanitizer and UBSan (tests/cpp/split_route_levels_plan_main.cpp): for every model in {0, 1, 3}, route in
{0, 1, 3, 5, 7, 13, 15}, dimension, residual_only, phase, scheme, material, layout and lattice (box, sub-box, level lattice of the
overlay), every plan of routes 0 to 7 equals the parent commit's rule field by field, routes 13 and 15 are 5 and 7 everywhere but in
the full model-3 split assembly of a level lattice, and there the plan is supported with voldev_jac, rows_residual == pair ==
false, PFM_RES_3 and k_cart_split3_jac over the tiles of k_cart_uu3 on that level's lattice.  Built like
tests/test_split_route_jacobian_plan_host.py builds its program: hipcc, host pass only, the sanitizers on the host pass; no HIP
call, no GPU, not loaded into Python."""
import os
import subprocess

import pytest

from test_cart_plan_host import HDR_DIR, ROOT, SWITCHES, _hipcc

SRC = os.path.join(ROOT, "tests", "cpp", "split_route_levels_plan_main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("split_route_levels_plan") / "split_route_levels_plan_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [cc, "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "-I" + HDR_DIR]
    for f in san:
        cmd += ["-Xarch_host", f]
    subprocess.check_call(cmd + ["-c", SRC, "-o", exe + ".o"])
    subprocess.check_call([cc] + san + [exe + ".o", "-o", exe])
    return exe


def test_the_full_assembly_of_a_level_lattice_is_the_one_new_plan(program):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([program], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "split_route_levels_plan: OK" in r.stdout and "FAIL" not in r.stdout
