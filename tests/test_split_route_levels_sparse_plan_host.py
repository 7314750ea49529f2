"""PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE / _ALL_LEVELS_SPARSE (61, 63) in the plan of a cartesian assembly
(cracks_amd/csrc/pfm_cart_plan.h: CartPlan::voldev_sparse on a level lattice; pfm_set_split_route) as a stand-alone host program
under AddressSanitizer and UBSan (tests/cpp/split_route_levels_sparse_plan_main.cpp): the truth table of plan_cart over route
{0, 5, 13, 15, 21, 23, 61, 63} x model x split x box / sub-box / level lattice x residual-only / full.  voldev_sparse is set on a
level lattice exactly for 61 / 63 under model 3 with the split on in a full assembly; the plans of all older routes equal the
parent commit's rule field by field.  Built like tests/test_split_route_sparse_plan_host.py builds its program: hipcc, host pass
only, the sanitizers on the host pass; no HIP call, no GPU, not loaded into Python."""
import os
import subprocess

import pytest

from test_cart_plan_host import HDR_DIR, ROOT, SWITCHES, _hipcc

SRC = os.path.join(ROOT, "tests", "cpp", "split_route_levels_sparse_plan_main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("split_route_levels_sparse_plan") / "split_route_levels_sparse_plan_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [cc, "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "-I" + HDR_DIR]
    for f in san:
        cmd += ["-Xarch_host", f]
    subprocess.check_call(cmd + ["-c", SRC, "-o", exe + ".o"])
    subprocess.check_call([cc] + san + [exe + ".o", "-o", exe])
    return exe


def test_voldev_sparse_on_a_level_lattice_needs_bits_8_16_and_32_and_older_routes_keep_their_plans(program):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([program], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "split_route_levels_sparse_plan: OK" in r.stdout and "FAIL" not in r.stdout
