"""CPU: the N > 1 path over torch.distributed (gloo), world_size 2, 4 and 8 (every grid is forced in turn: world 8
includes the 2 x 4 grid of BASELINE configs[2])."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.parametrize("world", [2, 4, 8])
def test_engines_over_gloo(world):
    env = dict(os.environ)
    env.pop("RP_SPMM_REIDX", None)
    env["OMP_NUM_THREADS"] = "1"
    # the ranks work on host buffers and must neither see nor open a GPU, also on a machine that has one: with a device
    # visible the communicator stages its payloads through HIP, and the library pins its host buffers, so all ranks
    # would open the device.  HIP_VISIBLE_DEVICES hides the devices; GPU_ENABLE_PAL=1 makes the HIP runtime skip its
    # ROCm device layer (Linux builds have no PAL layer), so it reports no device without opening one -- the library's
    # path for a machine without a GPU runtime, as on a CPU-only machine
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["GPU_ENABLE_PAL"] = "1"
    port = 29600 + world
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_WORKER_OK world=%d" % world in r.stdout
