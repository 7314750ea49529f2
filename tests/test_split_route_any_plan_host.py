"""PFM_SPLIT_ROUTE_LATTICE_ANY in the plan of a cartesian assembly (cracks_amd/csrc/pfm_cart_plan.h: CartPlan::spectral next to
CartPlan::voldev) as a stand-alone host program under AddressSanitizer and UBSan (tests/cpp/split_route_any_plan_main.cpp):
the spectral plan -- model 1 on route 3, the residual-only assembly of a 3-D lattice with the split on -- equals the voldev plan
of the same lattice and phase in every field but the law, model 3 on route 3 is model 3 on route 1, and every other combination
is what plan_cart answers without the argument.  Built like tests/test_split_route_plan_host.py builds its program: hipcc, host
pass only, the sanitizers on the host pass; no HIP call, no GPU, not loaded into Python."""
import os
import subprocess

import pytest

from test_cart_plan_host import HDR_DIR, ROOT, SWITCHES, _hipcc

SRC = os.path.join(ROOT, "tests", "cpp", "split_route_any_plan_main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("split_route_any_plan") / "split_route_any_plan_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [cc, "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "-I" + HDR_DIR]
    for f in san:
        cmd += ["-Xarch_host", f]
    subprocess.check_call(cmd + ["-c", SRC, "-o", exe + ".o"])
    subprocess.check_call([cc] + san + [exe + ".o", "-o", exe])
    return exe


def test_the_spectral_plan_is_the_voldev_plan_but_for_the_law(program):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([program], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "split_route_any_plan: OK" in r.stdout and "FAIL" not in r.stdout
