"""GPU: update_values, update_values_dev, exec_t, exec_t_f32 and sddmm of the 2D engine on degenerate grids
(tests/gpu_dist_para2d_layouts_worker.py): a rectangular A whose B blocks differ from its panels, runs of odd length at odd
offsets, a slice of one row, an empty slice, a grid row without rows of A, one without rows of B, grid columns without a column --
every entry bit for bit against exact data, with 2 and 4 ranks sharing the card (exchange staged through the host) or, on a node
with a GPU per rank, over RCCL."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "gpu_dist_para2d_layouts_worker.py")


def _launch(world, port, native):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    if native:
        env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        env["CRPSPMM_EXPECT_NATIVE_RCCL"] = "1"
        env.pop("CRPSPMM_EXCHANGE", None)
    else:
        env["CRPSPMM_EXCHANGE"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), WORKER]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_PARA2D_LAYOUTS_WORKER_OK world=%d" % world in r.stdout


@pytest.mark.parametrize("world", [2, 4])
def test_para2d_layouts_multi_rank_one_gpu(world):
    _launch(world, 29920 + world, native=False)


def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.parametrize("world", [2, 4])
def test_para2d_layouts_native_rccl_multi_gpu(world):
    """The same worker with one rank per GPU and the native RCCL exchange; skipped on a box with fewer GPUs, as
    tests/test_gpu_engine_layouts.py::test_layouts_native_rccl_multi_gpu is."""
    if _gpu_count() < world:
        pytest.skip("needs %d GPUs (native RCCL refuses two ranks on one device)" % world)
    _launch(world, 29930 + world, native=True)
