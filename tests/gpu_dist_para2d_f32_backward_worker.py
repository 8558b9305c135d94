"""Worker for tests/test_gpu_f32_backward.py: the 2D engine's fp32 transposed product and its device-resident value updates on
every pm x pn grid of N ranks, a grid row with an empty A0 slice included -- sharing ONE GPU with device payloads staged
through the host (the rehearsal mode of tests/gpu_dist_para2d_ops_worker.py), or with a GPU per rank and the native RCCL
exchange.  Every rank's block of C := A^T * B meets the entrywise fp32 bound of tests/fp32_ref.py against the GLOBAL
transpose; a twin engine updated from the host gives the same bits as the one whose slices are all-gathered between device
buffers, from fp64 and from fp32 values.  CRP_TEST_HOST_GATHER=1 (with CRPSPMM_REPLICATE=host): the short form of the run --
one matrix, n = 7 -- in which the slices are gathered through allgatherv_bytes on host copies."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def np_transpose(rp, ci, va, ncol):
    order = np.argsort(ci, kind="stable")
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncol))]).astype(np.int32)
    return rp_t, rows[order].astype(np.int32), va[order]


def run_grid(ctx, pm, pn, a0, ac, n, mat, data, tag):
    import torch
    import torch.distributed as dist
    fp32_ref, engine, planner, world, dev = ctx
    rp, ci, va, rp_t = mat
    Y32, B32, ref, bound, v_new, v_new32 = data
    me = world.rank
    pi, pj = me // pn, me % pn
    bc = planner.even_displs(n, pn)
    c0, c1 = int(bc[pj]), int(bc[pj + 1])
    r0, r1 = int(ac[pi]), int(ac[pi + 1])
    n_loc = c1 - c0
    mine = slice(int(rp[a0[me]]), int(rp[a0[me + 1]]))                # this rank's slice of the global nonzeros
    snz = mine.stop - mine.start
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def run(call, shape, tdt):
        out = torch.full(shape, float("nan"), dtype=tdt, device=dev)
        call(out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), (me, tag)
        return got

    mk = lambda: engine.Para2dSpmm(world, pm, pn, a0, ac, ac, bc, rp[a0[me]:a0[me + 1] + 1], ci[mine], va[mine])
    e2, twin = mk(), mk()
    assert e2.slice_nnz == snz, (me, tag)
    Yd, Bd = T(Y32[r0:r1, c0:c1]), T(B32[r0:r1, c0:c1])
    Y64, B64 = T(Y32[r0:r1, c0:c1].astype(np.float64)), T(B32[r0:r1, c0:c1].astype(np.float64))
    blk = (r1 - r0, n_loc)

    # ---- exec_t_f32: the bound against the global transpose, the inner engine bit for bit, both timing modes
    fwd = run(lambda o: e2.exec(0, Bd, o), blk, torch.float32)
    assert not e2.rp.transposed_built, (me, tag)
    seq = run(lambda o: e2.exec_t_f32(0, Yd, o), blk, torch.float32)
    assert e2.rp.transposed_built, (me, tag)
    fp32_ref.check_f32_bound(rp_t[r0:r1 + 1], None, None, None, seq, what="rank %d %s exec_t_f32" % (me, tag),
                             ref_bound=(ref[r0:r1, c0:c1], bound[r0:r1, c0:c1]))
    assert np.array_equal(run(lambda o: e2.rp.exec_t_f32(0, Yd, o), blk, torch.float32), seq), (me, tag, "inner engine")
    e2.rp.set_timing(False)
    for rep in range(3):
        assert np.array_equal(run(lambda o: e2.exec_t_f32(0, Yd, o), blk, torch.float32), seq), (me, tag, rep, "timing off")
    assert np.array_equal(run(lambda o: e2.exec(0, Bd, o), blk, torch.float32), fwd), (me, tag, "forward after exec_t_f32")
    e2.rp.set_timing(True)

    # ---- update_values_dev in both dtypes against the twin's host update
    def products(g):
        return [("exec", run(lambda o: g.exec(0, B64, o), blk, torch.float64)),
                ("exec f32", run(lambda o: g.exec(0, Bd, o), blk, torch.float32)),
                ("exec_t", run(lambda o: g.exec_t(0, Y64, o), blk, torch.float64)),
                ("exec_t_f32", run(lambda o: g.exec_t_f32(0, Yd, o), blk, torch.float32)),
                ("sddmm", run(lambda o: g.sddmm(0, Y64, B64, o, mode=1), (snz,), torch.float64))]

    before = products(e2)
    e2.update_values_dev(T(v_new[mine]))
    twin.update_values(v_new[mine])
    assert e2.rp.host_values_stale == (e2.rp.nnz() > 0) and not twin.rp.host_values_stale, (me, tag)
    after = products(e2)
    for (what, a), (_w, b) in zip(after, products(twin)):
        assert np.array_equal(a, b), (me, tag, what, "update_values_dev differs from update_values")
    if e2.rp.nnz() > 0 and blk[0] > 0:
        assert not np.array_equal(after[0][1], before[0][1]), (me, tag, "the update changed nothing")
    e2.update_values_dev(T(v_new32[mine]))
    twin.update_values(v_new32[mine].astype(np.float64))
    for (what, a), (_w, b) in zip(products(e2), products(twin)):
        assert np.array_equal(a, b), (me, tag, what, "fp32 values")
    # the panel's values behind the plan: the row's slices in rank order
    p0, p1 = int(rp[a0[pi * pn]]), int(rp[a0[(pi + 1) * pn]])
    assert np.array_equal(e2.rp.plan()["A_val"], v_new32[p0:p1].astype(np.float64)) and not e2.rp.host_values_stale, (me, tag, "host mirror")
    e2.free()
    twin.free()
    dist.barrier()


def main():
    import torch
    import torch.distributed as dist
    import fp32_ref
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
    ctx = (fp32_ref, engine, planner, world, dev)
    m = 6000
    rng = np.random.default_rng(41)                                   # the same stream on every rank
    rp_b, ci_b, va_b = gen.banded_fem(m, offsets=(1, 2, 3, 4, 50, 51, 1400), seed=5)
    rp_r, ci_r, va_r = gen.random_csr(m, m, 30)
    mats = [("banded_fem", rp_b, ci_b, fp32_ref.data_values(rng, va_b.size)),             # A != A^T: independent values
            ("random_csr", rp_r, ci_r, fp32_ref.data_values(rng, va_r.size))]
    first = None
    short = os.environ.get("CRP_TEST_HOST_GATHER") == "1"
    if short:
        assert os.environ.get("CRPSPMM_REPLICATE") == "host"
    for name, rp, ci, va in mats[:1] if short else mats:
        rp_t, ci_t, va_t = np_transpose(rp, ci, va, m)
        rb = planner.csr_mat_row_partition(rp, P)
        for n in (7,) if short else (7, 256):
            Y32, B32 = fp32_ref.data_B(rng, (m, n)), fp32_ref.data_B(rng, (m, n))
            ref, bound = fp32_ref.f32_bound(rp_t, ci_t, va_t, Y32)
            data = (Y32, B32, ref, bound, fp32_ref.data_values(rng, va.size), fp32_ref.data_values(rng, va.size).astype(np.float32))
            mat = (rp, ci, va, rp_t)
            if first is None:
                first = (mat, data, n, name)
            for pn in [d for d in range(1, P + 1) if P % d == 0]:
                pm = P // pn
                ac = np.array([rb[i * pn] for i in range(pm + 1)], dtype=np.int32)
                a0 = np.zeros(P + 1, dtype=np.int32)
                for i in range(pm):
                    loc = rp[ac[i]:ac[i + 1] + 1] - rp[ac[i]]
                    a0[i * pn:(i + 1) * pn + 1] = planner.csr_mat_row_partition(loc, pn) + ac[i]
                run_grid(ctx, pm, pn, a0, ac, n, mat, data, "%s %dx%d n=%d" % (name, pm, pn, n))
    # a grid row whose first rank holds no rows of A0: pm x 2, A0_rowptr by hand
    mat, data, n, name = first
    pn, pm = 2, P // 2
    ac = np.array([m * i // pm for i in range(pm + 1)], dtype=np.int32)
    a0 = np.zeros(P + 1, dtype=np.int32)
    for i in range(pm):
        a0[2 * i], a0[2 * i + 1] = ac[i], (ac[i] + ac[i + 1]) // 2
    a0[0:2] = ac[0]
    a0[P] = m
    run_grid(ctx, pm, pn, a0, ac, n, mat, data, "%s %dx2 empty slice n=%d" % (name, pm, n))
    if me == 0:
        print("GPU_DIST_PARA2D_F32_BACKWARD_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
