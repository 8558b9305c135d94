"""Worker for tests/test_sddmm.py: one process per rank, gloo backend, CPU only.  The data flow of the row-parallel engine's
SDDMM replayed in numpy from the plans of plan-only engines: Y is packed by rB_sridxs, the rows move by the plan's counts and
displacements through the communicator (host buffers), and the dots are formed through crp_rp_spmm_dev_colidx_host -- the
kernel's role is played by numpy.  The operands hold small integers, so every dot is exact and the comparison with the global
SDDMM is entry for entry, in the order of A_val."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def small_ints(seed, shape):
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float64)


def replay(plan, comm, X_loc, Y_loc, n, mode):
    P = plan["nproc"]
    send = np.ascontiguousarray(Y_loc[plan["rB_sridxs"], :n]).reshape(-1)          # 1. pack by the forward plan's send list
    if send.size == 0:
        send = np.zeros(1)
    nrecv = int(plan["rB_rdispls"][P])
    recv = np.full(max(nrecv, 1), np.nan)
    ll = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_longlong))
    sc, sd, rc, rd = (np.ascontiguousarray(plan[k], dtype=np.int64) for k in ("rB_scnts", "rB_sdispls", "rB_rcnts", "rB_rdispls"))
    comm.struct.alltoallv_dev_f64(None, send.ctypes.data, ll(sc), ll(sd), recv.ctypes.data, ll(rc), ll(rd), None)   # 2. exchange
    Y1 = recv[:nrecv].reshape(-1, n)
    code = plan["dev_colidx"].astype(np.int64)                                        # 3. dots through the two-source code
    rows = np.repeat(np.arange(plan["A_nrow"]), np.diff(plan["A_rowptr"]))
    yrows = np.where((code >= 0)[:, None], Y_loc[np.where(code >= 0, code, 0)], Y1[np.where(code < 0, ~code, 0)] if nrecv else 0.0)
    out = np.einsum("ij,ij->i", X_loc[rows], yrows)
    return out * plan["A_val"] if mode else out


def main():
    import torch.distributed as dist
    from crp_spmm_amd import comm as crp_comm, engine, gen, planner

    crp_comm.init_process_group()
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    m = k = 6000
    n = 24
    rp_b, ci_b, va_b = gen.banded_fem(m, offsets=(1, 2, 3, 4, 50, 51, 1400), seed=5)
    for name, (rp, ci, va) in (("banded_fem", (rp_b, ci_b, va_b)), ("random_csr", gen.random_csr(m, k, 30))):
        va = small_ints(3, va.size)
        X, Y = small_ints(1, (m, n)), small_ints(2, (k, n))
        grow = np.repeat(np.arange(m), np.diff(rp))
        want = np.einsum("ij,ij->i", X[grow], Y[ci])                                 # the global SDDMM
        rb = planner.csr_mat_row_partition(rp, P)
        s, e = int(rb[me]), int(rb[me + 1])
        eng = engine.RpSpmm(s, e - s, rp[s:e + 1], ci[rp[s]:rp[e]], va[rp[s]:rp[e]], rb, n, world, plan_only=True)
        plan = eng.plan()
        assert (plan["dev_colidx"] < 0).any() and (plan["dev_colidx"] >= 0).any(), (me, name, "both sources are in use")
        for mode in (0, 1):
            got = replay(plan, world, X[s:e], Y[s:e], n, mode)
            ref = want[rp[s]:rp[e]] * (va[rp[s]:rp[e]] if mode else 1.0)
            assert got.shape == ref.shape and np.array_equal(got, ref), (me, name, mode)
        eng.free()
        dist.barrier()
    if me == 0:
        print("DIST_SDDMM_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
