"""Worker for tests/test_gpu_attention.py: the row-parallel engine's fused attention on N ranks that share ONE GPU, device
payloads staged through the host (the rehearsal mode of tests/gpu_dist_worker.py).  Every rank forms the FULL matrix's O, lse
and p_out with the device-level call on one handle and asserts that its engine's results are those arrays' slices bit for bit, in
both dtypes, with and without the values as bias, timing on and off.  Three layouts: the balanced partition, under which at
least one rank's engine is split into interior and boundary rows; one in which a rank holds no rows of A; one in which a rank
holds no rows of B (of K and V)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist
    from crp_spmm_amd import comm as crp_comm, engine, gen, hip, planner

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    crp_comm.init_process_group(device=None)
    assert crp_comm.exchange_mode() == "host"
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    m = k = 400
    cases = (("banded_fem", gen.banded_fem(m, offsets=(1, 2, 3, 4, 10, 11, 30), seed=5), 24),
             ("random_csr", gen.random_csr(m, k, 30, empty_every=13), 7))
    for name, (rp, ci, va), n in cases:
        rp = rp.astype(np.int32)
        va = np.random.default_rng(3).uniform(-2, 2, ci.size)
        bal = np.array(planner.csr_mat_row_partition(rp, P))
        hole = bal.copy()
        hole[1] = hole[0] if P == 2 else hole[2]                      # P == 2: rank 0 without rows; else rank 1
        A = hip.CsrDev(m, k, rp, ci, va)
        for layout, rb, bd in (("balanced", bal, bal), ("a rank without rows of A", hole, bal), ("a rank without rows of B", bal, hole)):
            s0, e0 = int(rb[me]), int(rb[me + 1])
            b0, b1 = int(bd[me]), int(bd[me + 1])
            lo, hi = int(rp[s0]), int(rp[e0])
            eng = engine.RpSpmm(s0, e0 - s0, rp[s0:e0 + 1], ci[lo:hi], va[lo:hi], bd, n, world)
            flags = torch.tensor([int(sum(eng.overlap_rows()) > 0), int(e0 == s0), int(b1 == b0)], device=dev)
            dist.all_reduce(flags)
            if layout == "balanced":
                assert int(flags[0]) > 0, "no rank's engine is split"
            elif layout == "a rank without rows of A":
                assert int(flags[1]) > 0, "every rank holds rows of A"
            else:
                assert int(flags[2]) > 0, "every rank holds rows of B"
            assert eng.nnz() == hi - lo and not eng.attention_built()
            for ndt in (np.float64, np.float32):
                rng = np.random.default_rng(17)
                Q, K, V = (rng.standard_normal(sh).astype(ndt) for sh in ((m, n), (k, n), (k, n)))
                Qd, Kd, Vd = T(Q), T(K), T(V)
                scale = 1.0 / np.sqrt(n)
                for bias in (False, True):
                    lse_f = torch.full((m,), float("nan"), dtype=Qd.dtype, device=dev)
                    p_f = torch.full((ci.size,), float("nan"), dtype=Qd.dtype, device=dev)
                    O_f = A.attention(Qd, Kd, Vd, scale=scale, bias=bias, lse=lse_f, p_out=p_f)
                    torch.cuda.synchronize()
                    want = (O_f.cpu().numpy()[s0:e0], lse_f.cpu().numpy()[s0:e0], p_f.cpu().numpy()[lo:hi])
                    for timing in (True, False):
                        eng.set_timing(timing)
                        O = torch.full((e0 - s0, n), float("nan"), dtype=Qd.dtype, device=dev)
                        lse = torch.full((e0 - s0,), float("nan"), dtype=Qd.dtype, device=dev)
                        p = torch.full((hi - lo,), float("nan"), dtype=Qd.dtype, device=dev)
                        eng.attention(0, Qd[s0:e0], Kd[b0:b1], Vd[b0:b1], O, scale=scale, bias=bias, lse=lse, p_out=p)
                        torch.cuda.synchronize()
                        assert eng.attention_built(), (me, name, layout)                 # also on a rank without rows
                        what = (me, name, layout, ndt.__name__, bias, timing)
                        assert np.array_equal(O.cpu().numpy(), want[0]), (what, "O")
                        assert np.array_equal(lse.cpu().numpy(), want[1]), (what, "lse")
                        assert np.array_equal(p.cpu().numpy(), want[2]), (what, "p_out")
            eng.free()
            dist.barrier()
        A.free()
    if me == 0:
        print("GPU_DIST_ATTENTION_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
