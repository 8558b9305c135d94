"""Worker for tests/test_gpu_streams.py: every call of the row-parallel engine and of the 2D engine (grids 2 x 1 and 1 x 2) made on
a non-blocking side stream, on two ranks that share ONE GPU with device payloads staged through the host, and compared bit for bit
with the same call on the default stream.  The balanced partition splits at least one rank's engine into interior and boundary
rows, so the calls take the `xstream` paths with a caller stream that is not the null stream.

What this proves and what it does not: the host-staged exchange synchronises the stream it is given, so these runs show that the
non-null `s` paths WORK (every kernel, copy and event is given a usable stream and the results are the default stream's), not
that they are ORDERED -- a missing wait between the caller's stream and the exchange stream would be hidden by the staging.  The
order of the overlap path is checked on the host (tests/host_engine_streams.cpp) and stays unchecked on several real devices."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist
    import crp_spmm_amd
    from crp_spmm_amd import comm as crp_comm, engine, gen, planner
    from streams_harness import bits

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    crp_comm.init_process_group(device=None)
    assert crp_comm.exchange_mode() == "host"
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    assert P == 2
    lib = crp_spmm_amd.load()
    sp = C.c_void_p()
    assert lib.crp_stream_create(C.byref(sp)) == 0
    S = torch.cuda.ExternalStream(sp.value)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rnd = lambda seed, shape, dt: T(np.random.default_rng(seed).standard_normal(shape).astype(dt))
    tdt = {np.float64: torch.float64, np.float32: torch.float32}

    def both(what, call, outs):
        """the call on the default stream, then on the side stream: the same bits"""
        for t in outs:
            t.fill_(float("nan"))
        call()
        torch.cuda.synchronize()
        want = [bits(t) for t in outs]
        assert not any(np.isnan(t.cpu().numpy()).any() for t in outs), (me, what, "NaN on the default stream")
        with torch.cuda.stream(S):
            for t in outs:
                t.fill_(float("nan"))
            call()
        S.synchronize()
        torch.cuda.synchronize()
        for t, w in zip(outs, want):
            assert np.array_equal(bits(t), w), (me, what, "the side stream's result differs")

    m = k = 400
    n = 24
    rp, ci, va = gen.banded_fem(m, offsets=(1, 2, 3, 4, 10, 11, 30), seed=5)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    va = np.random.default_rng(3).uniform(-2, 2, ci.size)
    bal = np.array(planner.csr_mat_row_partition(rp, P))
    s0, e0 = int(bal[me]), int(bal[me + 1])
    lo, hi = int(rp[s0]), int(rp[e0])
    rows, nnz = e0 - s0, hi - lo

    # ---- the row-parallel engine, timing off
    eng = engine.RpSpmm(s0, rows, rp[s0:e0 + 1], ci[lo:hi], va[lo:hi], bal, n, world)
    eng.set_timing(False)
    flag = torch.tensor([int(sum(eng.overlap_rows()) > 0)], device=dev)
    dist.all_reduce(flag)
    assert int(flag[0]) > 0, "no rank's engine is split"
    newv = T(np.random.default_rng(4).uniform(-2, 2, nnz))
    for ndt in (np.float64, np.float32):
        dt = tdt[ndt]
        name = np.dtype(ndt).name
        Bm, X = rnd(1, (rows, n), ndt), rnd(2, (rows, n), ndt)
        C_, Ct = torch.empty((rows, n), dtype=dt, device=dev), torch.empty((rows, n), dtype=dt, device=dev)
        both("exec " + name, lambda: eng.exec(0, Bm, C_), [C_])
        both("exec_t " + name, lambda: (eng.exec_t if ndt is np.float64 else eng.exec_t_f32)(0, X, Ct), [Ct])
        out = torch.empty((nnz,), dtype=dt, device=dev)
        for mode in (0, 1):
            both("sddmm %s mode %d" % (name, mode), lambda: eng.sddmm(0, X, Bm, out, mode=mode), [out])
        s, dy = rnd(3, (nnz,), ndt), rnd(4, (nnz,), ndt)
        both("row_softmax " + name, lambda: eng.row_softmax(s, out=out), [out])
        both("row_softmax_bwd " + name, lambda: eng.row_softmax_bwd(s, dy, out=out), [out])
        Q, Kk, V, dO = (rnd(5 + i, (rows, n), ndt) for i in range(4))
        O, lse, p = torch.empty((rows, n), dtype=dt, device=dev), torch.empty((rows,), dtype=dt, device=dev), torch.empty((nnz,), dtype=dt, device=dev)
        both("attention " + name, lambda: eng.attention(0, Q, Kk, V, O, scale=0.2, bias=True, lse=lse, p_out=p), [O, lse, p])
        O0, lse0 = O.clone(), lse.clone()
        dQ, dK, dV = (torch.empty((rows, n), dtype=dt, device=dev) for _ in range(3))
        ds = torch.empty((nnz,), dtype=dt, device=dev)
        both("attention_bwd " + name, lambda: eng.attention_bwd(Q, Kk, V, O0, dO, lse0, dQ, dK, dV, scale=0.2, bias=True, ds_out=ds),
             [dQ, dK, dV, ds])
        # two heads of 12 columns: the multi-head attention and its backward, the GAT and the GATv2 forward
        hd = 2
        lse2, p2 = torch.empty((rows, hd), dtype=dt, device=dev), torch.empty((nnz, hd), dtype=dt, device=dev)
        both("attention heads 2 " + name, lambda: eng.attention(0, Q, Kk, V, O, scale=0.2, bias=True, lse=lse2, p_out=p2, heads=hd),
             [O, lse2, p2])
        O1, lse1 = O.clone(), lse2.clone()
        ds2 = torch.empty((nnz, hd), dtype=dt, device=dev)
        both("attention_bwd heads 2 " + name,
             lambda: eng.attention_bwd(Q, Kk, V, O1, dO, lse1, dQ, dK, dV, scale=0.2, bias=True, ds_out=ds2, heads=hd), [dQ, dK, dV, ds2])
        el, er, av = rnd(21, (rows, hd), ndt), rnd(22, (rows, hd), ndt), rnd(23, (hd, n // hd), ndt)
        both("gat_attention heads 2 " + name, lambda: eng.gat_attention(0, el, er, V, O, slope=0.2, bias=True, lse=lse2, p_out=p2, heads=hd),
             [O, lse2, p2])
        both("gatv2_attention heads 2 " + name,
             lambda: eng.gatv2_attention(0, Q, av, Kk, O, slope=0.2, bias=True, lse=lse2, p_out=p2, heads=hd), [O, lse2, p2])
        vals = newv.to(dt)
        both("update_values_dev %s, exec" % name, lambda: (eng.update_values_dev(vals), eng.exec(0, Bm, C_)), [C_])
    torch.cuda.synchronize()
    eng.free()
    dist.barrier()

    # ---- the 2D engine on both grids of two ranks
    for pm, pn in ((2, 1), (1, 2)):
        ac = np.array([bal[i * pn] for i in range(pm + 1)], dtype=np.int32)
        a0 = np.zeros(P + 1, dtype=np.int32)
        for i in range(pm):
            loc = rp[ac[i]:ac[i + 1] + 1] - rp[ac[i]]
            a0[i * pn:(i + 1) * pn + 1] = np.array(planner.csr_mat_row_partition(loc, pn)) + ac[i]
        pi, pj = me // pn, me % pn
        bc = planner.even_displs(n, pn)
        n_loc = int(bc[pj + 1] - bc[pj])
        r = int(ac[pi + 1] - ac[pi])
        a, b = int(a0[me]), int(a0[me + 1])
        my = (rp[a:b + 1], ci[rp[a]:rp[b]], va[rp[a]:rp[b]])
        e2 = engine.Para2dSpmm(world, pm, pn, a0, ac, ac, bc, *my)
        e2.rp.set_timing(False)
        snz = e2.slice_nnz
        tag = "%d x %d" % (pm, pn)
        for ndt in (np.float64, np.float32):
            dt = tdt[ndt]
            name = "%s %s" % (tag, np.dtype(ndt).name)
            Bm, X = rnd(11, (r, n_loc), ndt), rnd(12, (r, n_loc), ndt)
            C_ = torch.empty((r, n_loc), dtype=dt, device=dev)
            both("2D exec " + name, lambda: e2.exec(0, Bm, C_), [C_])
            both("2D exec_t " + name, lambda: (e2.exec_t if ndt is np.float64 else e2.exec_t_f32)(0, X, C_), [C_])
            out = torch.empty((snz,), dtype=dt, device=dev)
            for mode in (0, 1):
                both("2D sddmm %s mode %d" % (name, mode), lambda: e2.sddmm(0, X, Bm, out, mode=mode), [out])
            s, dy = rnd(13, (snz,), ndt), rnd(14, (snz,), ndt)
            if snz:
                both("2D row_softmax " + name, lambda: e2.row_softmax(s, out=out), [out])
                both("2D row_softmax_bwd " + name, lambda: e2.row_softmax_bwd(s, dy, out=out), [out])
            vals = T(np.random.default_rng(15).uniform(-2, 2, snz).astype(ndt))
            both("2D update_values_dev %s, exec" % name, lambda: (e2.update_values_dev(vals), e2.exec(0, Bm, C_)), [C_])
        torch.cuda.synchronize()
        e2.free()
        dist.barrier()
    torch.cuda.synchronize()
    lib.crp_stream_destroy(sp)
    if me == 0:
        print("GPU_DIST_STREAMS_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
