"""CPU: the rank layouts of tests/gpu_dist_layouts_worker.py without a GPU -- plan-only engines over torch.distributed (gloo) at
world 2 and 4: plan() against oracle.rp_plan_all on every partition (a rank without rows of A, without rows of B, one rank
owning all of B, unrelated partitions of a rectangular A), and the product emulated from the plan against exact data."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.parametrize("world", [2, 4])
def test_layout_plans_over_gloo(world):
    env = dict(os.environ)
    env.pop("RP_SPMM_REIDX", None)
    env["OMP_NUM_THREADS"] = "1"
    # the ranks must neither see nor open a GPU (tests/test_dist_cpu.py)
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["GPU_ENABLE_PAL"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29620 + world),
           os.path.join(ROOT, "tests", "gpu_dist_layouts_worker.py"), "--plan-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_LAYOUTS_PLAN_OK world=%d" % world in r.stdout
