"""Worker for tests/test_gpu_attention_mh_dist.py: the row-parallel engine's multi-head attention and its backward
(RpSpmm.attention / attention_bwd with ``heads``) on N ranks that share ONE GPU, device payloads staged through the host (the
rehearsal mode of tests/gpu_dist_worker.py).  Every rank forms the FULL matrix's multi-head forward and backward with the
device-level calls on one pair of handles and asserts that its engine's O, lse, p_out, dQ and ds_out are those arrays' slices bit
for bit -- timing on and off, repeated calls -- that dK and dV are bit-identical over repeats and timing modes, equal the handle
call at one rank and, across ranks, lie inside the bound the single-head worker uses for them (attention_bwd_ref per head), and
that an exec before and after gives the same bits.  glb_n = 64 in 4 heads, both dtypes, with and without the values as bias.
Layouts: the balanced partition (with more than one rank at least one engine is split into interior and boundary rows), a rank
without rows of A, a rank without rows of B.  Last, in fp64, glb_n = 520 in 2 heads: the single-head backward refuses that width,
the multi-head one serves it."""
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
    nan = lambda dt, *shape: torch.full(shape, float("nan"), dtype=dt, device=dev)
    m = k = 400
    rp, ci, _ = gen.banded_fem(m, offsets=(1, 2, 3, 4, 10, 11, 30), seed=5)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    nnz = ci.size
    va = np.random.default_rng(3).uniform(-2, 2, nnz)
    bal = np.array(planner.csr_mat_row_partition(rp, P))
    layouts = [("balanced", bal, bal)]
    if P > 1:
        hole = bal.copy()
        hole[1] = hole[0] if P == 2 else hole[2]                      # P == 2: rank 0 without rows; else rank 1
        layouts += [("a rank without rows of A", hole, bal), ("a rank without rows of B", bal, hole)]
    A = hip.CsrDev(m, k, rp, ci, va)
    At = hip.CsrDev.from_transpose(m, k, rp, ci, va)

    def whole(Qd, Kd, Vd, dOd, H, scale, bias):
        """the handle's multi-head calls on the whole matrix"""
        lse, p, ds = nan(Qd.dtype, m, H), nan(Qd.dtype, nnz, H), nan(Qd.dtype, nnz, H)
        O = A.attention(Qd, Kd, Vd, scale=scale, bias=bias, lse=lse, p_out=p, heads=H)
        dQ, delta = A.attention_bwd_q(Qd, Kd, Vd, O, dOd, lse, scale=scale, bias=bias, ds_out=ds, heads=H)
        dK, dV = At.attention_bwd_kv(Kd, Vd, Qd, dOd, lse, delta, scale=scale, bias=bias, heads=H)
        torch.cuda.synchronize()
        return dict(O=O, lse=lse, p=p, dQ=dQ, ds=ds, dK=dK, dV=dV)

    def engine_calls(eng, full, Qd, Kd, Vd, dOd, H, scale, bias, rows, brows, nz, what, forward=True):
        """the engine's calls, timing on, off and off again, against the slices of `full`; returns this rank's (dK, dV)"""
        (s0, e0), (b0, b1), (lo, hi) = rows, brows, nz
        n = Qd.shape[1]
        first = None
        for timing in (True, False, False):
            eng.set_timing(timing)
            if forward:
                O, lse, p = nan(Qd.dtype, e0 - s0, n), nan(Qd.dtype, e0 - s0, H), nan(Qd.dtype, hi - lo, H)
                eng.attention(0, Qd[s0:e0], Kd[b0:b1], Vd[b0:b1], O, scale=scale, bias=bias, lse=lse, p_out=p, heads=H)
                torch.cuda.synchronize()
                assert eng.attention_built(), what
                assert torch.equal(O, full["O"][s0:e0]), (what, timing, "O")
                assert torch.equal(lse, full["lse"][s0:e0]), (what, timing, "lse")
                assert torch.equal(p, full["p"][lo:hi]), (what, timing, "p_out")
            dQ, ds = nan(Qd.dtype, e0 - s0, n), nan(Qd.dtype, hi - lo, H)
            dK, dV = nan(Qd.dtype, b1 - b0, n), nan(Qd.dtype, b1 - b0, n)
            eng.attention_bwd(Qd[s0:e0], Kd[b0:b1], Vd[b0:b1], full["O"][s0:e0], dOd[s0:e0], full["lse"][s0:e0], dQ, dK, dV, scale=scale,
                              bias=bias, ds_out=ds, heads=H)
            torch.cuda.synchronize()
            assert eng.attention_bwd_built(), what                  # also on a rank without rows
            assert torch.equal(dQ, full["dQ"][s0:e0]), (what, timing, "dQ")
            assert torch.equal(ds, full["ds"][lo:hi]), (what, timing, "ds_out")
            if first is None:
                first = (dK, dV)
            assert torch.equal(dK, first[0]) and torch.equal(dV, first[1]), (what, timing, "dK, dV repeat")
        if P == 1:
            assert torch.equal(first[0], full["dK"]) and torch.equal(first[1], full["dV"]), (what, "dK, dV at one rank")
        return first

    def inside_the_bound(first, refs, H, d, ndt, brows, what):
        """dK and dV per head against the np.longdouble reference, as tests/gpu_dist_attention_bwd_worker.py holds them (its
        argument for the bound across ranks stands per head)"""
        b0, b1 = brows
        for h in range(H):
            for kk, arr, bnd in (("dK", first[0], B.bound_dK), ("dV", first[1], B.bound_dV)):
                got = arr.cpu().numpy()[:, h * d:(h + 1) * d]
                assert np.isfinite(got).all(), (what, kk, h)
                tol = np.asarray(bnd(refs[h], ndt))[b0:b1]
                err = np.abs(got.astype(np.longdouble) - refs[h][kk][b0:b1])
                assert (err <= tol).all(), (what, kk, h, float((err / np.where(tol > 0, tol, 1)).max()))

    def references(Q, K, V, dO, H, d, scale, bias, ndt):
        return [B.reference(rp, ci, *(x[:, h * d:(h + 1) * d] for x in (Q, K, V, dO)), scale, va.astype(ndt) if bias else None)
                for h in range(H)]

    n, H = 64, 4
    d = n // H
    data, fulls, refs = {}, {}, {}
    for ndt in (np.float64, np.float32):
        rng = np.random.default_rng(17)
        Q, K, V, dO, Bm = (rng.standard_normal(sh).astype(ndt) for sh in ((m, n), (k, n), (k, n), (m, n), (k, n)))
        scale = float(ndt(1.0 / np.sqrt(d)))
        data[ndt] = (Q, K, V, dO, T(Q), T(K), T(V), T(dO), T(Bm), scale)
        for bias in (False, True):
            fulls[ndt, bias] = whole(*data[ndt][4:8], H, scale, bias)
            if P > 1:
                refs[ndt, bias] = references(Q, K, V, dO, H, d, scale, bias, ndt)
    for layout, rb, bd in layouts:
        rows, brows = (int(rb[me]), int(rb[me + 1])), (int(bd[me]), int(bd[me + 1]))
        nz = (int(rp[rows[0]]), int(rp[rows[1]]))
        eng = engine.RpSpmm(rows[0], rows[1] - rows[0], rp[rows[0]:rows[1] + 1], ci[nz[0]:nz[1]], va[nz[0]:nz[1]], bd, n, world)
        flags = torch.tensor([int(sum(eng.overlap_rows()) > 0), int(rows[1] == rows[0]), int(brows[1] == brows[0])], device=dev)
        dist.all_reduce(flags)
        if layout == "balanced":
            assert P == 1 or int(flags[0]) > 0, "no rank's engine is split"
        elif layout == "a rank without rows of A":
            assert int(flags[1]) > 0, "every rank holds rows of A"
        else:
            assert int(flags[2]) > 0, "every rank holds rows of B"
        assert not eng.attention_built() and not eng.attention_bwd_built()
        for ndt in (np.float64, np.float32):
            Q, K, V, dO, Qd, Kd, Vd, dOd, Bd, scale = data[ndt]
            C0 = nan(Qd.dtype, rows[1] - rows[0], n)
            eng.exec(0, Bd[brows[0]:brows[1]], C0)
            torch.cuda.synchronize()
            for bias in (False, True):
                what = (me, layout, ndt.__name__, bias)
                first = engine_calls(eng, fulls[ndt, bias], Qd, Kd, Vd, dOd, H, scale, bias, rows, brows, nz, what)
                if P > 1:
                    inside_the_bound(first, refs[ndt, bias], H, d, ndt, brows, what)
            C1 = nan(Qd.dtype, rows[1] - rows[0], n)
            eng.exec(0, Bd[brows[0]:brows[1]], C1)
            torch.cuda.synchronize()
            assert torch.equal(C0, C1) and bool(C0.isfinite().all()), (me, layout, ndt.__name__, "an exec before and after")
        eng.free()
        dist.barrier()

    # fp64, 520 columns: over the backward's cap as one head, 260 per head in two
    n, H = 520, 2
    d = n // H
    rng = np.random.default_rng(23)
    Q, K, V, dO = (rng.standard_normal(sh) for sh in ((m, n), (k, n), (k, n), (m, n)))
    scale = float(1.0 / np.sqrt(d))
    Qd, Kd, Vd, dOd = T(Q), T(K), T(V), T(dO)
    full = whole(Qd, Kd, Vd, dOd, H, scale, True)
    rows = brows = (int(bal[me]), int(bal[me + 1]))
    nz = (int(rp[rows[0]]), int(rp[rows[1]]))
    eng = engine.RpSpmm(rows[0], rows[1] - rows[0], rp[rows[0]:rows[1] + 1], ci[nz[0]:nz[1]], va[nz[0]:nz[1]], bal, n, world)
    outs = [nan(Qd.dtype, rows[1] - rows[0], n), nan(Qd.dtype, brows[1] - brows[0], n), nan(Qd.dtype, brows[1] - brows[0], n)]
    try:
        eng.attention_bwd(Qd[rows[0]:rows[1]], Kd[brows[0]:brows[1]], Vd[brows[0]:brows[1]], full["O"][rows[0]:rows[1]], dOd[rows[0]:rows[1]],
                          full["lse"][rows[0]:rows[1], 0].contiguous(), *outs, scale=scale)
        raise AssertionError("the single-head backward took 520 fp64 columns")
    except ValueError:
        pass
    assert not eng.attention_bwd_built()
    what = (me, "520 columns in 2 heads")
    first = engine_calls(eng, full, Qd, Kd, Vd, dOd, H, scale, True, rows, brows, nz, what, forward=False)
    if P > 1:
        inside_the_bound(first, references(Q, K, V, dO, H, d, scale, True, np.float64), H, d, np.float64, brows, what)
    eng.free()
    dist.barrier()
    A.free()
    At.free()
    if me == 0:
        print("GPU_DIST_ATTENTION_MH_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
