"""Worker for tests/test_gpu_para2d_ops.py: value updates, C := A^T*B and SDDMM of the 2D engine on every pm x pn grid of N
ranks -- sharing ONE GPU with device payloads staged through the host (the rehearsal mode of tests/gpu_dist_t_worker.py),
or with a GPU per rank and the native RCCL exchange.  Every rank holds its A0 slice, and the blocks of the dense operands
its grid position owns; the SDDMM's partial dots over the rank's column slice are reduce-scattered along the grid row and
come out in the order of the rank's own slice."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_TOL = 1e-12            # the project's fp64 bar: relative Frobenius error against the oracle
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
# the lines of crp_para2d_spmm_print_stat, as they were before this engine could do more than A*B
STAT_LINES = ("para2d_spmm_init() time =", "Total comm size for replicating A =", "Total comm size for replicating B =",
              "Total comm size for SpMM          =", "-------------------- Runtime (s) --------------------",
              "                                     avg         max", "Replicate A matrix (once)        ",
              "Pack B matrix for redistribution ", "Redistribute B matrix            ", "Unpack received B matrix data    ",
              "Local SpMM                       ", "Total para2d_spmm_exec()         ", "Replicate A + para2d_spmm_exec() ")


def np_transpose(rp, ci, va, ncol):
    order = np.argsort(ci, kind="stable")
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncol))]).astype(np.int32)
    return rp_t, rows[order].astype(np.int32), va[order]


def slices(rp, ci, va, displs, r):
    s, e = displs[r], displs[r + 1]
    return rp[s:e + 1], ci[rp[s]:rp[e]], va[rp[s]:rp[e]]


def small_ints(seed, shape):
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float64)


def captured_stdout(fn):
    """What fn() writes to file descriptor 1 (the library prints with printf and flushes)."""
    sys.stdout.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(1)
        os.dup2(f.fileno(), 1)
        try:
            fn()
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        f.seek(0)
        return f.read().decode()


def run_grid(ctx, pm, pn, a0, ac, n, rp, ci, va, tag, check_stat):
    import torch
    import torch.distributed as dist
    orc, engine, planner, world, dev = ctx
    me = world.rank
    pi, pj = me // pn, me % pn
    m = rp.size - 1
    bc = planner.even_displs(n, pn)
    c0, c1 = int(bc[pj]), int(bc[pj + 1])
    r0, r1 = int(ac[pi]), int(ac[pi + 1])
    n_loc, nj_max = c1 - c0, int(np.diff(bc).max())
    my = slices(rp, ci, va, a0, me)
    s0, s1 = int(rp[a0[me]]), int(rp[a0[me + 1]])                  # this rank's slice of the global nonzeros
    snz = s1 - s0
    grow = np.repeat(np.arange(m), np.diff(rp))[s0:s1]
    gcol = ci[s0:s1]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    e2 = engine.Para2dSpmm(world, pm, pn, a0, ac, ac, bc, *my)
    assert e2.slice_nnz == snz and not e2.sddmm_built, (me, tag)

    # ---- forward, and laziness: an exec-only engine has built nothing and prints the lines it always printed
    B = orc.fill_B(0, m, 0, n)
    C_ref = orc.spmm_csr(rp, ci, va, B)[r0:r1, c0:c1]
    Bd = T(B[r0:r1, c0:c1])
    Cd = torch.full((r1 - r0, n_loc), float("nan"), dtype=torch.float64, device=dev)
    e2.exec(0, Bd, Cd)
    torch.cuda.synchronize()
    assert orc.rel_fro_err(C_ref, Cd.cpu().numpy()) <= FP64_TOL, (me, tag, "exec")
    assert not e2.sddmm_built and not e2.rp.sddmm_built and not e2.rp.transposed_built, (me, tag)
    if check_stat:
        text = captured_stdout(e2.print_stat)
        if me == 0:
            lines = [ln for ln in text.splitlines() if ln.strip()]
            assert len(lines) == len(STAT_LINES) and all(ln.startswith(w.rstrip()) for ln, w in zip(lines, STAT_LINES)), text

    # ---- C := A^T * B: against the oracle's product with the numpy-transposed matrix, and the inner engine bit for bit
    Yt = orc.fill_B(0, m, 0, n, fi=0.23, fj=0.11)
    Ct_ref = orc.spmm_csr(*np_transpose(rp, ci, va, m), Yt)[r0:r1, c0:c1]
    Yd = T(Yt[r0:r1, c0:c1])
    Ctd = torch.full((r1 - r0, n_loc), float("nan"), dtype=torch.float64, device=dev)
    e2.exec_t(0, Yd, Ctd)
    torch.cuda.synchronize()
    Ct = Ctd.cpu().numpy().copy()
    assert orc.rel_fro_err(Ct_ref, Ct) <= FP64_TOL, (me, tag, "exec_t", orc.rel_fro_err(Ct_ref, Ct))
    Ctd.fill_(float("nan"))
    e2.rp.exec_t(0, Yd, Ctd)
    torch.cuda.synchronize()
    assert np.array_equal(Ctd.cpu().numpy(), Ct), (me, tag, "exec_t differs from the inner engine's")
    assert not e2.sddmm_built, (me, tag)

    # ---- SDDMM on rounded data: every entry against long double, by the derived bound; bit-identity across timing modes
    rng = np.random.default_rng(100 + n)
    X64, Y64 = rng.standard_normal((m, n)), rng.standard_normal((m, n))
    first = True
    for tdt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        X, Y = X64.astype(ndt), Y64.astype(ndt)
        Xd, Yd2 = T(X[r0:r1, c0:c1]), T(Y[r0:r1, c0:c1])
        prod = X[grow].astype(np.longdouble) * Y[gcol].astype(np.longdouble)
        ref0, S0 = prod.sum(axis=1), np.abs(prod).sum(axis=1)
        val = my[2].astype(ndt).astype(np.longdouble)               # the engine's values as stored in this dtype
        out = torch.empty(snz, dtype=tdt, device=dev)
        for mode in (0, 1):
            e2.rp.set_timing(True)
            out.fill_(float("nan"))
            e2.sddmm(0, Xd, Yd2, out, mode=mode)
            torch.cuda.synchronize()
            if first:
                assert e2.sddmm_built == (pn > 1), (me, tag)
                first = False
            got = out.cpu().numpy().copy()
            assert not np.isnan(got).any(), (me, tag, ndt.__name__, mode)
            ref, S, k = (ref0 * val, S0 * np.abs(val), nj_max + pn + 1) if mode else (ref0, S0, nj_max + pn)
            err = np.abs(got.astype(np.longdouble) - ref)
            bound = 1.0001 * k * U[ndt] * S
            assert (err <= bound).all(), (me, tag, ndt.__name__, mode, "worst err / bound", float((err / bound).max()))
            e2.rp.set_timing(False)
            for rep in range(3):
                out.fill_(float("nan"))
                e2.sddmm(0, Xd, Yd2, out, mode=mode)
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), got), (me, tag, ndt.__name__, mode, rep, "timing off differs from timing on")
        # host operands, column-major, host out: the same bits (one dtype per width, so that both are met)
        if (ndt is np.float64) == (n == 10):
            e2.rp.set_timing(True)
            oh = np.full(snz, np.nan, ndt)
            e2.sddmm(1, np.ascontiguousarray(X[r0:r1, c0:c1].T), np.ascontiguousarray(Y[r0:r1, c0:c1].T), oh, mode=1)
            assert not np.isnan(oh).any() and np.array_equal(oh, got), (me, tag, ndt.__name__, "host operands, layout 1")

    # ---- update_values(2 * values): exec and exec_t double
    e2.rp.set_timing(True)
    e2.update_values(2.0 * my[2])
    e2.exec(0, Bd, Cd)
    torch.cuda.synchronize()
    assert orc.rel_fro_err(2.0 * C_ref, Cd.cpu().numpy()) <= FP64_TOL, (me, tag, "exec after update_values")
    e2.exec_t(0, T(Yt[r0:r1, c0:c1]), Ctd)
    torch.cuda.synchronize()
    assert orc.rel_fro_err(2.0 * Ct_ref, Ctd.cpu().numpy()) <= FP64_TOL, (me, tag, "exec_t after update_values")

    # ---- SDDMM on exact data: small integers in X, Y and the values, every dot exact in fp32 and fp64 -- the integer
    #      reference in the order of the rank's slice, no tolerance: a wrong offset, segment or order shows
    vi = small_ints(3, va.size)
    Xi, Yi = small_ints(1, (m, n)), small_ints(2, (m, n))
    want0 = np.einsum("ij,ij->i", Xi[grow], Yi[gcol])
    e2.update_values(vi[s0:s1])
    for tdt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        Xd, Yd2 = T(Xi[r0:r1, c0:c1].astype(ndt)), T(Yi[r0:r1, c0:c1].astype(ndt))
        longer = torch.full((snz + 1,), float("nan"), dtype=tdt, device=dev)      # one entry longer: the sentinel stays
        longer[snz] = 12345.0
        for mode, timing in ((0, False), (1, True)):
            e2.rp.set_timing(timing)
            longer[:snz] = float("nan")
            e2.sddmm(0, Xd, Yd2, longer[:snz], mode=mode)
            torch.cuda.synchronize()
            got = longer.cpu().numpy()
            assert got[snz] == 12345.0, (me, tag, ndt.__name__, mode, "wrote past the slice")
            want = (want0 * vi[s0:s1] if mode else want0).astype(ndt)
            assert np.array_equal(got[:snz], want), (me, tag, ndt.__name__, mode, "exact data")
        e2.update_values(2.0 * vi[s0:s1])
        e2.sddmm(0, Xd, Yd2, longer[:snz], mode=1)
        torch.cuda.synchronize()
        assert np.array_equal(longer.cpu().numpy()[:snz], (2.0 * want0 * vi[s0:s1]).astype(ndt)), (me, tag, ndt.__name__, "doubled values")
        e2.update_values(vi[s0:s1])

    # ---- the original values restored
    e2.update_values(my[2])
    e2.exec(0, Bd, Cd)
    torch.cuda.synchronize()
    assert orc.rel_fro_err(C_ref, Cd.cpu().numpy()) <= FP64_TOL, (me, tag, "exec after the values were restored")
    e2.free()
    dist.barrier()


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
    ctx = (orc, engine, planner, world, dev)
    m = 1200
    rp_b, ci_b, va_b = gen.banded_fem(m, offsets=(1, 2, 3, 40, 41, 500))
    va_b = va_b * (1.0 + 0.37 * np.sin(np.arange(va_b.size)))            # A != A^T
    mats = (("banded_fem", (rp_b, ci_b, va_b)), ("random_csr", gen.random_csr(m, m, 9)))
    for name, (rp, ci, va) in mats:
        rb = planner.csr_mat_row_partition(rp, P)
        for pn in [d for d in range(1, P + 1) if P % d == 0]:
            pm = P // pn
            ac = np.array([rb[i * pn] for i in range(pm + 1)], dtype=np.int32)
            a0 = np.zeros(P + 1, dtype=np.int32)
            for i in range(pm):
                loc = rp[ac[i]:ac[i + 1] + 1] - rp[ac[i]]
                a0[i * pn:(i + 1) * pn + 1] = planner.csr_mat_row_partition(loc, pn) + ac[i]
            for n in (10, 50):
                run_grid(ctx, pm, pn, a0, ac, n, rp, ci, va, "%s %dx%d n=%d" % (name, pm, pn, n), check_stat=(n == 10))
    # a grid row whose first rank holds no rows of A0: pm x 2, A0_rowptr by hand
    name, (rp, ci, va) = mats[0]
    pn, pm = 2, P // 2
    ac = np.array([m * i // pm for i in range(pm + 1)], dtype=np.int32)
    a0 = np.zeros(P + 1, dtype=np.int32)
    for i in range(pm):
        a0[2 * i], a0[2 * i + 1] = ac[i], (ac[i] + ac[i + 1]) // 2
    a0[0:2] = ac[0]
    a0[P] = m
    run_grid(ctx, pm, pn, a0, ac, 10, rp, ci, va, "%s %dx2 empty slice n=10" % (name, pm), check_stat=False)
    if me == 0:
        print("GPU_DIST_PARA2D_OPS_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
