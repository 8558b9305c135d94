"""CPU: the grids of tests/gpu_dist_para2d_layouts_worker.py without a GPU -- plan-only 2D engines over torch.distributed (gloo) at
world 2 and 4: the slice counts against A0_rowptr, the value update against the panel's concatenation, and the SDDMM's data flow
replayed in numpy on exact data, equal to the expected `out` entry for entry; a negative control reads every run from an even
offset and must not pass; and grids() itself, whose asserts say what every grid is there for."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.parametrize("world", [2, 4])
def test_para2d_layout_plans_over_gloo(world):
    env = dict(os.environ)
    env.pop("RP_SPMM_REIDX", None)
    env["OMP_NUM_THREADS"] = "1"
    # the ranks must neither see nor open a GPU (tests/test_dist_cpu.py)
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["GPU_ENABLE_PAL"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29640 + world),
           os.path.join(ROOT, "tests", "gpu_dist_para2d_layouts_worker.py"), "--plan-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_PARA2D_LAYOUTS_PLAN_OK world=%d" % world in r.stdout


def test_grids_reach_what_they_are_for():
    """grids() for 2 and 4 ranks on all three matrices: its own asserts (monotone displacements, the panels' first rows, and the
    property of every grid), the grid names per (pm, pn), and the run offsets of grid `odd`."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_para2d_layouts_worker as w
    from crp_spmm_amd import gen, planner
    mats = w.matrices(gen)
    assert [x[0] for x in mats] == ["band", "rect", "lower"]
    for name, rp, ci, m, k in mats:
        for P, count in ((2, 7), (4, 13)):
            gs = w.grids(planner, rp, m, k, P)
            assert len(gs) == count, (name, P, [(g[0], g[1], g[2]) for g in gs])
            for pn in (d for d in range(1, P + 1) if P % d == 0):
                pm = P // pn
                want = ["bal"] + (["odd", "one", "none"] if pn >= 2 else []) + (["nopanel", "noB"] if pm >= 2 else [])
                assert [g[0] for g in gs if g[2] == pn] == want, (name, P, pn)
            for gname, pm, pn, a0, br, ac in gs:
                off = w.run_offsets(rp, a0, pm, pn)
                assert off.shape == (pm, pn + 1) and (off[:, 0] == 0).all() and off[:, pn].sum() == rp[-1], (name, P, gname)
                if gname == "odd":
                    assert ((off[:, 1:pn] % 2 == 1) | (off[:, 1:pn] == off[:, pn:])).all(), (name, P, pn, off)
                if gname == "nopanel":
                    assert (off[1] == 0).all(), (name, P, pn, off)
                if gname == "noB":
                    assert br[1] == 0 and k > 0, (name, P, pn, br)
            assert [g[0] for g in w.grids_of(planner, "lower", rp, m, k, P)] == ["bal"] * sum(1 for d in range(1, P + 1) if P % d == 0)
