"""PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE / _ALL_SPARSE in the plan of a cartesian assembly (cracks_amd/csrc/pfm_cart_plan.h:
CartPlan::voldev_sparse; pfm_set_split_route) as a stand-alone host program under AddressSanitizer and UBSan
(tests/cpp/split_route_sparse_plan_main.cpp): over the product of tests/cpp/split_route_jacobian_plan_main.cpp with the routes
{0 ... 15, 21, 23}, voldev_sparse is set exactly where voldev_jac is set, the route has bit 16 and the lattice is no level
lattice; the plans of 21 / 23 equal those of 5 / 7 in every other field; every plan of the routes 0 ... 15 equals the parent
commit's rule field by field.  Built like tests/test_split_route_jacobian_plan_host.py builds its program: hipcc, host pass
only, the sanitizers on the host pass; no HIP call, no GPU, not loaded into Python."""
import os
import subprocess

import pytest

from test_cart_plan_host import HDR_DIR, ROOT, SWITCHES, _hipcc

SRC = os.path.join(ROOT, "tests", "cpp", "split_route_sparse_plan_main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("split_route_sparse_plan") / "split_route_sparse_plan_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [cc, "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "-I" + HDR_DIR]
    for f in san:
        cmd += ["-Xarch_host", f]
    subprocess.check_call(cmd + ["-c", SRC, "-o", exe + ".o"])
    subprocess.check_call([cc] + san + [exe + ".o", "-o", exe])
    return exe


def test_voldev_sparse_is_the_one_new_field_and_routes_0_to_15_keep_their_plans(program):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([program], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "split_route_sparse_plan: OK" in r.stdout and "FAIL" not in r.stdout
