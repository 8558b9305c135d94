"""CPU: the rank layouts of tests/gpu_dist_layouts_worker.py without a GPU -- plan-only engines over torch.distributed (gloo) at
world 2 and 4: plan() against oracle.rp_plan_all on every partition (a rank without rows of A, without rows of B, one rank
owning all of B, unrelated partitions of a rectangular A), and the product emulated from the plan against exact data; and
the worker's data for the transposed product and the SDDMM, whose generators assert their exactness budgets."""
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


def test_transposed_and_sddmm_data_keep_their_budgets():
    """Data.exact_t_sets and Data.sddmm_set for every matrix and width: the budget asserts of fp64_ref.exact_parts and
    fp32_ref.exact_problem32 on the transposed pattern, the values carried back to A's order, and the SDDMM set's own asserts."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_layouts_worker as w
    from crp_spmm_amd import gen
    for name, rp, ci, m, k in w.matrices(gen):
        data = w.Data(name, rp, ci, m, k)
        rp_t, ci_t, order = data.transposed()
        assert rp_t.size == k + 1 and rp_t[-1] == rp[-1] and np.array_equal(np.sort(order), np.arange(rp[-1]))
        rows = np.repeat(np.arange(m), np.diff(rp))
        for n in w.WIDTHS:
            for what, val, B, C_exact in data.exact_t_sets(n):
                assert val.shape == (rp[-1],) and B.shape == (m, n) and C_exact.shape == (k, n), (name, n, what)
                # the values in A's order give the same product through A's own pattern: C[c] += val[p] * B[row(p)]
                C = np.zeros((k, n))
                np.add.at(C, ci[:rp[-1]], val[:, None] * B[rows].astype(np.float64))
                assert np.array_equal(C, C_exact.astype(np.float64)), (name, n, what)
            val, X, Y, out0, out1 = data.sddmm_set(n)
            assert X.shape == (m, n) and Y.shape == (k, n) and val.shape == out0.shape == out1.shape == (rp[-1],), (name, n)
            assert np.array_equal((X[rows] * Y[ci[:rp[-1]]]).sum(axis=1), out0) and np.array_equal(out0 * val, out1), (name, n)
