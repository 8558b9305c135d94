"""Worker for tests/test_gpu_row_softmax.py: the row-parallel engine's row softmax and its backward on N ranks -- sharing ONE
GPU with device payloads staged through the host (the rehearsal mode of tests/gpu_dist_worker.py), or with a GPU per rank and
the native RCCL exchange.  Every rank forms the FULL matrix's result with the device-level call and asserts that its engine's
result is that array's slice bit for bit, in both dtypes.  Two layouts: the balanced row partition, under which at least one
rank's engine is split into interior and boundary rows, and one in which a rank holds no rows of A."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist
    import softmax_ref as R
    from crp_spmm_amd import comm as crp_comm, engine, gen, hip, planner

    native = os.environ.get("CRPSPMM_EXPECT_NATIVE_RCCL") == "1"
    idev = int(os.environ.get("LOCAL_RANK", "0")) if native else 0
    torch.cuda.set_device(idev)
    dev = torch.device("cuda", idev)
    crp_comm.init_process_group(device=idev if native else None)
    assert crp_comm.exchange_mode() == ("nccl" if native else "host")
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    m = k = 3000
    rp_b, ci_b, va_b = gen.banded_fem(m, offsets=(1, 2, 3, 4, 50, 51, 700), seed=5)
    n = 8
    for name, (rp, ci, va) in (("banded_fem", (rp_b, ci_b, va_b)), ("random_csr", gen.random_csr(m, k, 30, empty_every=13))):
        rp = rp.astype(np.int32)
        bal = planner.csr_mat_row_partition(rp, P)
        hole = np.array(bal)
        hole[1] = hole[0] if P == 2 else hole[2]                      # P == 2: rank 0 without rows; else rank 1
        for layout, rb in (("balanced", bal), ("a rank without rows", hole)):
            s0, e0 = int(rb[me]), int(rb[me + 1])
            lo, hi = int(rp[s0]), int(rp[e0])
            eng = engine.RpSpmm(s0, e0 - s0, rp[s0:e0 + 1], ci[lo:hi], va[lo:hi], bal, n, world)
            split = torch.tensor([int(sum(eng.overlap_rows()) > 0), int(e0 == s0)], device=dev)
            dist.all_reduce(split)
            if layout == "balanced":
                assert int(split[0]) > 0, "no rank's engine is split"
            else:
                assert int(split[1]) > 0, "every rank holds rows"
            assert eng.nnz() == hi - lo and not eng.row_softmax_built
            for ndt in (np.float64, np.float32):
                s = R.scores(rp, ndt, 8, 31)
                dy = R.grads(s.size, ndt, 32)
                rp_d, s_d, dy_d = T(rp), T(s), T(dy)
                full = hip.row_softmax(rp_d, s_d)
                full_b = hip.row_softmax_bwd(rp_d, full, dy_d)
                torch.cuda.synchronize()
                want, want_b = full.cpu().numpy()[lo:hi], full_b.cpu().numpy()[lo:hi]
                out = torch.full((hi - lo,), float("nan"), dtype=s_d.dtype, device=dev)
                assert eng.row_softmax(s_d[lo:hi].clone(), out=out) is out
                torch.cuda.synchronize()
                assert eng.row_softmax_built, (me, name, layout)                 # also on the rank without rows
                assert np.array_equal(out.cpu().numpy(), want), (me, name, layout, ndt.__name__, "forward")
                got = eng.row_softmax_bwd(out, dy_d[lo:hi].clone())
                torch.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy(), want_b), (me, name, layout, ndt.__name__, "backward")
                t = s_d[lo:hi].clone()
                eng.row_softmax(t, out=t)
                torch.cuda.synchronize()
                assert np.array_equal(t.cpu().numpy(), want), (me, name, layout, ndt.__name__, "in place")
            eng.free()
            dist.barrier()
    if me == 0:
        print("GPU_DIST_SOFTMAX_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
