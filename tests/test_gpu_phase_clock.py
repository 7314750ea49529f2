"""The phase clocks of k_cart_uu3 and k_cart_phi4 (PFM_UU_CLK, PFM_PHI_CLK; profiling, tools/profile_round.sh): the clocked
instantiations compute what the plain ones compute, the report lines arrive on stderr with plausible numbers, and a layout the
clocks are not instantiated for runs unclocked.  The variables are read once per process: one process per mode, two
assemblies in each (the second reuses the context's counter buffer)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import TOL, linf_scaled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CLOCKS = ("PFM_UU_CLK", "PFM_PHI_CLK")
SCRIPT = (
    "import sys, numpy as np\n"
    f"sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]\n"
    "import test_gpu_cart as T\n"
    "from gpu_util import make_context\n"
    "c = T.box_case(*T.BOXES[1], sys.argv[2] == 'blocked')\n"
    "ctx = make_context(c)\n"
    "out = []\n"
    "for _ in range(2):\n"
    "    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)\n"
    "    out += [np.ravel(v) for v in values] + [res]\n"
    "ctx.close()\n"
    "np.save(sys.argv[1], np.concatenate(out))\n")


def _run(tmp, layout, env):
    script = tmp / "run.py"
    script.write_text(SCRIPT)
    f = tmp / "out.npy"
    e = {k: v for k, v in os.environ.items() if k not in CLOCKS}
    e.update(env)
    r = subprocess.run([sys.executable, str(script), str(f), layout], env=e, timeout=600, capture_output=True, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr
    return np.load(f), [ln for ln in r.stderr.splitlines() if "phase clock" in ln]


@pytest.fixture(scope="module")
def default_run(tmp_path_factory):
    got = {}

    def get(layout):
        if layout not in got:
            got[layout], lines = _run(tmp_path_factory.mktemp("default_" + layout), layout, {})
            assert lines == []
        return got[layout]

    return get


def _fields(line):
    """every `name=value` of a report line, and the `Wn a/b` pairs of the per-wave line"""
    vals = re.findall(r"=([^\s\]]+)", line)
    for a, b in re.findall(r"W\d (\S+)/(\S+)", line):
        vals += [a, b]
    return [float(x) for x in vals]


@pytest.mark.parametrize("var,value,tag,lines_per_launch",
                         [("PFM_UU_CLK", "1", "[k_cart_uu3 phase clock", 3), ("PFM_PHI_CLK", "1", "[k_cart_phi4 phase clock", 1),
                          ("PFM_PHI_CLK", "2", "[k_cart_phi4 phase clock", 1)])
def test_clocked_kernels_compute_the_same_and_report(tmp_path, default_run, var, value, tag, lines_per_launch):
    want = default_run("blocked")
    got, lines = _run(tmp_path, "blocked", {var: value})
    assert got.shape == want.shape and linf_scaled(got, want) < TOL
    assert len(lines) == 2 * lines_per_launch and all(ln.startswith(tag) for ln in lines), lines
    assert ("role 3 up to" in lines[0]) == (value == "2")
    for ln in lines:
        f = _fields(ln)
        assert f and all(math.isfinite(x) and x >= 0.0 for x in f), ln


def test_interleaved_layout_runs_unclocked(tmp_path, default_run):
    """the clocked forms exist for the blocked layout only: the plan says so, and the launch is the plain one"""
    want = default_run("interleaved")
    got, lines = _run(tmp_path, "interleaved", {"PFM_PHI_CLK": "1"})
    assert got.shape == want.shape and linf_scaled(got, want) < TOL
    assert lines == []
