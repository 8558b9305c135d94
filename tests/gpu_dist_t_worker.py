"""Worker for tests/test_gpu_transpose.py: the row-parallel engine's transposed product C := A^T * B on N ranks -- sharing ONE
GPU with device payloads staged through the host (the rehearsal mode of tests/gpu_dist_worker.py), or with a GPU per rank
and the native RCCL exchange.  Every rank holds a row block of A and of B; the partial products of the rows other ranks own
travel back through the forward exchange plan run backwards and are added in a fixed order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def np_transpose(rp, ci, va, ncol):
    order = np.argsort(ci, kind="stable")
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncol))]).astype(np.int32)
    return rp_t, rows[order].astype(np.int32), va[order]


def main():
    import torch
    import torch.distributed as dist
    import oracle as orc
    from crp_spmm_amd import comm as crp_comm, engine, gen, planner

    native = os.environ.get("CRPSPMM_EXPECT_NATIVE_RCCL") == "1"
    idev = int(os.environ.get("LOCAL_RANK", "0")) if native else 0
    torch.cuda.set_device(idev)
    dev = torch.device("cuda", idev)
    crp_comm.init_process_group(device=idev if native else None)
    assert crp_comm.exchange_mode() == ("nccl" if native else "host")
    world = crp_comm.TorchComm()
    if native:
        assert world.device_ranks() == world.nproc, "the native RCCL communicator did not come up"
    P, me = world.nproc, world.rank
    m = k = 6000
    rp_b, ci_b, va_b = gen.banded_fem(m, offsets=(1, 2, 3, 4, 50, 51, 1400), seed=5)
    va_b = va_b * (1.0 + 0.37 * np.sin(np.arange(va_b.size)))            # A != A^T
    for name, (rp, ci, va) in (("banded_fem", (rp_b, ci_b, va_b)), ("random_csr", gen.random_csr(m, k, 30))):
        rp_t, ci_t, va_t = np_transpose(rp, ci, va, k)
        rb = planner.csr_mat_row_partition(rp, P)
        s, e = int(rb[me]), int(rb[me + 1])
        for n in (24, 256):
            Y = orc.fill_B(0, m, 0, n, fi=0.23, fj=0.11)
            Ct_ref = orc.spmm_csr(rp_t, ci_t, va_t, Y)[s:e]               # this rank's rows of A^T Y
            B = orc.fill_B(0, k, 0, n)
            C_ref = orc.spmm_csr(rp, ci, va, B)[s:e]
            eng = engine.RpSpmm(s, e - s, rp[s:e + 1], ci[rp[s]:rp[e]], va[rp[s]:rp[e]], rb, n, world)
            Yd = torch.from_numpy(Y[s:e].copy()).to(dev)
            Bd = torch.from_numpy(B[s:e].copy()).to(dev)
            Cd = torch.full((e - s, n), float("nan"), dtype=torch.float64, device=dev)
            # ---- lazy build: a forward exec builds nothing transposed
            eng.exec(0, Bd, Cd)
            torch.cuda.synchronize()
            assert not eng.transposed_built, (me, name, n)
            # ---- parity, timing on: peers' part, exchange, local part, accumulate in sequence
            Cd.fill_(float("nan"))
            eng.exec_t(0, Yd, Cd)
            torch.cuda.synchronize()
            assert eng.transposed_built, (me, name, n)
            C_seq = Cd.cpu().numpy().copy()
            err = orc.rel_fro_err(Ct_ref, C_seq)
            assert err <= 1e-12, (me, name, n, "exec_t", err)
            # ---- overlap: timing off, the exchange beside the local product; no sum may change
            eng.set_timing(False)
            for rep in range(3):
                Cd.fill_(float("nan"))
                eng.exec_t(0, Yd, Cd)
                torch.cuda.synchronize()
                assert np.array_equal(Cd.cpu().numpy(), C_seq), (me, name, n, rep, "overlapped exec_t differs from the sequential one")
            # ---- forward unchanged: the exchange buffers are shared
            Cd.fill_(float("nan"))
            eng.exec(0, Bd, Cd)
            torch.cuda.synchronize()
            assert orc.rel_fro_err(C_ref, Cd.cpu().numpy()) <= 1e-12, (me, name, n, "forward after exec_t")
            # ---- value updates reach the transposed matrices
            eng.update_values(va[rp[s]:rp[e]] * 2.0)
            eng.exec_t(0, Yd, Cd)
            torch.cuda.synchronize()
            assert orc.rel_fro_err(2.0 * Ct_ref, Cd.cpu().numpy()) <= 1e-12, (me, name, n, "update_values")
            eng.exec(0, Bd, Cd)
            torch.cuda.synchronize()
            assert orc.rel_fro_err(2.0 * C_ref, Cd.cpu().numpy()) <= 1e-12, (me, name, n, "update_values, forward")
            eng.update_values(va[rp[s]:rp[e]])
            # ---- host pointers, column-major
            eng.set_timing(True)
            Ch = np.full((n, e - s), np.nan)
            eng.exec_t(1, np.ascontiguousarray(Y[s:e].T), Ch)
            assert orc.rel_fro_err(Ct_ref, Ch.T) <= 1e-12, (me, name, n, "exec_t host cm")
            eng.print_stat()
            eng.free()
            dist.barrier()
    if me == 0:
        print("GPU_DIST_T_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
