"""Worker for tests/test_gpu_attention_bwd.py: the row-parallel engine's fused attention backward on N ranks that share ONE GPU,
device payloads staged through the host (the rehearsal mode of tests/gpu_dist_worker.py).  Every rank forms the FULL matrix's
forward and backward with the device-level calls on one pair of handles and asserts that its engine's dQ and ds_out are those
arrays' slices bit for bit, that its dK and dV are inside the derived bounds against the np.longdouble reference
(tests/attention_bwd_ref.py) and bit-identical over a repeated call and over timing on / off, in both dtypes, with and without the
values as bias.  Three layouts: the balanced partition, under which at least one rank's engine is split into interior and boundary
rows; one in which a rank holds no rows of A; one in which a rank holds no rows of B (of K and V)."""
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
    import attention_bwd_ref as B

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
        ci = ci.astype(np.int32)
        va = np.random.default_rng(3).uniform(-2, 2, ci.size)
        bal = np.array(planner.csr_mat_row_partition(rp, P))
        hole = bal.copy()
        hole[1] = hole[0] if P == 2 else hole[2]                      # P == 2: rank 0 without rows; else rank 1
        A = hip.CsrDev(m, k, rp, ci, va)
        refs = {}
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
            assert not eng.attention_bwd_built()
            for ndt in (np.float64, np.float32):
                rng = np.random.default_rng(17)
                Q, K, V, dO = (rng.standard_normal(sh).astype(ndt) for sh in ((m, n), (k, n), (k, n), (m, n)))
                Qd, Kd, Vd, dOd = T(Q), T(K), T(V), T(dO)
                scale = float(ndt(1.0 / np.sqrt(n)))
                for bias in (False, True):
                    key = (ndt, bias)
                    if key not in refs:
                        refs[key] = B.reference(rp, ci, Q, K, V, dO, scale, va.astype(ndt) if bias else None)
                    ref = refs[key]
                    lse_f = torch.full((m,), float("nan"), dtype=Qd.dtype, device=dev)
                    O_f = A.attention(Qd, Kd, Vd, scale=scale, bias=bias, lse=lse_f)
                    ds_f = torch.full((ci.size,), float("nan"), dtype=Qd.dtype, device=dev)
                    dQ_f, delta_f = A.attention_bwd_q(Qd, Kd, Vd, O_f, dOd, lse_f, scale=scale, bias=bias, ds_out=ds_f)
                    torch.cuda.synchronize()
                    first = None
                    for timing in (True, False, False):
                        eng.set_timing(timing)
                        dQ = torch.full((e0 - s0, n), float("nan"), dtype=Qd.dtype, device=dev)
                        dK = torch.full((b1 - b0, n), float("nan"), dtype=Qd.dtype, device=dev)
                        dV = torch.full((b1 - b0, n), float("nan"), dtype=Qd.dtype, device=dev)
                        ds = torch.full((hi - lo,), float("nan"), dtype=Qd.dtype, device=dev)
                        eng.attention_bwd(Qd[s0:e0], Kd[b0:b1], Vd[b0:b1], O_f[s0:e0], dOd[s0:e0], lse_f[s0:e0], dQ, dK, dV, scale=scale,
                                          bias=bias, ds_out=ds)
                        torch.cuda.synchronize()
                        assert eng.attention_bwd_built(), (me, name, layout)            # also on a rank without rows
                        what = (me, name, layout, ndt.__name__, bias, timing)
                        assert np.array_equal(dQ.cpu().numpy(), dQ_f.cpu().numpy()[s0:e0]), (what, "dQ")
                        assert np.array_equal(ds.cpu().numpy(), ds_f.cpu().numpy()[lo:hi]), (what, "ds_out")
                        got = (dK.cpu().numpy(), dV.cpu().numpy())
                        if first is None:
                            first = got
                        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), (what, "dK, dV repeat")
                    # dK and dV against the reference.  The bound holds across ranks as it stands: a column whose Lc entries lie on r
                    # ranks is summed in chains of L_1 .. L_r terms (each times scale) whose results are added one by one, at most
                    # max L_t + 1 + (r - 1) <= Lc + 1 roundings on any path, each relative to the sum of the absolute terms
                    for kk, arr, bnd in (("dK", first[0], B.bound_dK), ("dV", first[1], B.bound_dV)):
                        assert np.isfinite(arr).all(), (what, kk)
                        tol = np.asarray(bnd(ref, ndt))[b0:b1]
                        err = np.abs(arr.astype(np.longdouble) - ref[kk][b0:b1])
                        assert (err <= tol).all(), (what, kk, float((err / np.where(tol > 0, tol, 1)).max()))
            eng.free()
            dist.barrier()
        A.free()
    if me == 0:
        print("GPU_DIST_ATTENTION_BWD_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
