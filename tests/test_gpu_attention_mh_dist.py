"""GPU: the row-parallel engine's multi-head attention and its backward on 1, 2 and 4 ranks that share one GPU
(tests/gpu_dist_attention_mh_worker.py states what is held): bit-identical to the handle's multi-head calls on the whole matrix
across rank counts, timing modes and repeated calls, and the backward at 520 fp64 columns in 2 heads, which the single-head
engine call refuses."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [1, 2, 4])
def test_multi_rank_one_gpu(world):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    env.pop("CRPSPMM_EXPECT_NATIVE_RCCL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(30280 + world), os.path.join(ROOT, "tests", "gpu_dist_attention_mh_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_ATTENTION_MH_WORKER_OK world=%d" % world in r.stdout
