"""Worker for tests/test_gpu_sddmm.py: the row-parallel engine's SDDMM on N ranks -- sharing ONE GPU with device payloads
staged through the host (the rehearsal mode of tests/gpu_dist_worker.py), or with a GPU per rank and the native RCCL
exchange.  Every rank holds a row block of A, of X and of Y; the rows of Y its nonzeros name on other ranks arrive through
the forward exchange.  The ranks' outputs, concatenated in rank order, must equal the one-rank device-level result
(crp_sddmm_csr_f64 / _f32 on the whole matrix) BIT FOR BIT: every rank forms that result itself and compares its slice."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    from crp_spmm_amd import comm as crp_comm, engine, gen, hip, planner

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
    va_b = va_b * (1.0 + 0.37 * np.sin(np.arange(va_b.size)))
    for name, (rp, ci, va) in (("banded_fem", (rp_b, ci_b, va_b)), ("random_csr", gen.random_csr(m, k, 30))):
        rb = planner.csr_mat_row_partition(rp, P)
        s, e = int(rb[me]), int(rb[me + 1])
        lo, hi = int(rp[s]), int(rp[e])
        new_va = 2.0 * va + 1.0
        A = hip.CsrDev(m, k, rp, ci, va)
        for n in (24, 256):
            rng = np.random.default_rng(100 + n)
            X64, Y64 = rng.standard_normal((m, n)), rng.standard_normal((k, n))
            eng = engine.RpSpmm(s, e - s, rp[s:e + 1], ci[lo:hi], va[lo:hi], rb, n, world)
            assert not eng.sddmm_built, (me, name, n)
            for tdt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
                X, Y = X64.astype(ndt), Y64.astype(ndt)
                Xg, Yg = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
                Xd, Yd = torch.from_numpy(X[s:e].copy()).to(dev), torch.from_numpy(Y[s:e].copy()).to(dev)
                out = torch.empty(hi - lo, dtype=tdt, device=dev)
                for mode in (0, 1):
                    want = A.sddmm(Xg, Yg, mode=mode)
                    torch.cuda.synchronize()
                    want = want.cpu().numpy()[lo:hi]
                    # ---- timing on: pack, exchange, kernels in sequence
                    eng.set_timing(True)
                    out.fill_(float("nan"))
                    eng.sddmm(0, Xd, Yd, out, mode=mode)
                    torch.cuda.synchronize()
                    assert eng.sddmm_built
                    assert np.array_equal(out.cpu().numpy(), want), (me, name, n, ndt.__name__, mode, "sequential")
                    # ---- timing off: the interior rows' dots beside the exchange
                    eng.set_timing(False)
                    for rep in range(3):
                        out.fill_(float("nan"))
                        eng.sddmm(0, Xd, Yd, out, mode=mode)
                        torch.cuda.synchronize()
                        assert np.array_equal(out.cpu().numpy(), want), (me, name, n, ndt.__name__, mode, rep, "overlapped")
                    # ---- host operands, column-major, host out
                    eng.set_timing(True)
                    oh = np.full(hi - lo, np.nan, ndt)
                    eng.sddmm(1, np.ascontiguousarray(X[s:e].T), np.ascontiguousarray(Y[s:e].T), oh, mode=mode)
                    assert np.array_equal(oh, want), (me, name, n, ndt.__name__, mode, "host cm")
                # ---- mode 1 after a value update: the engine's parts and their fp32 copies follow
                eng.update_values(new_va[lo:hi])
                A.update_values(new_va)
                want = A.sddmm(Xg, Yg, mode=1)
                torch.cuda.synchronize()
                want = want.cpu().numpy()[lo:hi]
                for timing in (True, False):
                    eng.set_timing(timing)
                    out.fill_(float("nan"))
                    eng.sddmm(0, Xd, Yd, out, mode=1)
                    torch.cuda.synchronize()
                    assert np.array_equal(out.cpu().numpy(), want), (me, name, n, ndt.__name__, timing, "update_values")
                eng.update_values(va[lo:hi])
                A.update_values(va)
            eng.set_timing(True)
            eng.print_stat()
            eng.free()
            dist.barrier()
        A.free()
    if me == 0:
        print("GPU_DIST_SDDMM_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
