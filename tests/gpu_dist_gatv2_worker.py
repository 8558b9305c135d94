"""Worker for tests/test_gpu_gatv2_dist.py: the row-parallel engine's fused GATv2 attention (RpSpmm.gatv2_attention) on N ranks that
share ONE GPU, device payloads staged through the host (the rehearsal mode of tests/gpu_dist_worker.py).  Every rank forms the FULL
matrix's forward with the device-level call on one handle and asserts that its engine's O, lse and p_out are those arrays' slices
bit for bit -- timing on and off, repeated calls, H = 1 and 3 heads of glb_n = 24 columns, both dtypes, with and without the values
as bias; XS and O on the device and on the host in both layouts, lse and p_out on the host; ``gatv2_built`` reads False, then True;
an exec before and after gives the same bits; and the call on a non-blocking side stream gives the default stream's bits.  Layouts:
the balanced partition (with more than one rank at least one engine is split into interior and boundary rows), a rank without rows
of A, a rank without rows of B."""
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
    from crp_spmm_amd import comm as crp_comm, engine, gen, hip, planner
    from streams_harness import bits

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    crp_comm.init_process_group(device=None)
    assert crp_comm.exchange_mode() == "host"
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    lib = crp_spmm_amd.load()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nan = lambda dt, *shape: torch.full(shape, float("nan"), dtype=dt, device=dev)
    m = k = 400
    n = 24
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
    slope = 0.2

    data, fulls = {}, {}
    for ndt in (np.float64, np.float32):
        rng = np.random.default_rng(17)
        V, Bm = (rng.standard_normal((k, n)).astype(ndt) for _ in range(2))
        XT = rng.standard_normal((m, n)).astype(ndt)
        data[ndt] = dict(V=V, Vd=T(V), Bd=T(Bm))
        for H in (1, 3):
            av = (rng.standard_normal((H, n // H)) / np.sqrt(n // H)).astype(ndt)
            data[ndt][H] = (T(XT), T(av))
            for bias in (False, True):
                lse, p = nan(data[ndt]["Vd"].dtype, m, H), nan(data[ndt]["Vd"].dtype, nnz, H)
                O = A.gatv2_attention(T(XT), data[ndt]["Vd"], T(av), slope=slope, bias=bias, lse=lse, p_out=p, heads=H)
                torch.cuda.synchronize()
                assert bool(O.isfinite().all()) and bool(p.isfinite().all())
                fulls[ndt, H, bias] = dict(O=O, lse=lse, p=p)

    sp = C.c_void_p()
    assert lib.crp_stream_create(C.byref(sp)) == 0
    S = torch.cuda.ExternalStream(sp.value)

    for layout, rb, bd in layouts:
        (s0, e0), (b0, b1) = (int(rb[me]), int(rb[me + 1])), (int(bd[me]), int(bd[me + 1]))
        lo, hi = int(rp[s0]), int(rp[e0])
        eng = engine.RpSpmm(s0, e0 - s0, rp[s0:e0 + 1], ci[lo:hi], va[lo:hi], bd, n, world)
        flags = torch.tensor([int(sum(eng.overlap_rows()) > 0), int(e0 == s0), int(b1 == b0)], device=dev)
        dist.all_reduce(flags)
        if layout == "balanced":
            assert P == 1 or int(flags[0]) > 0, "no rank's engine is split"
        elif layout == "a rank without rows of A":
            assert int(flags[1]) > 0, "every rank holds rows of A"
        else:
            assert int(flags[2]) > 0, "every rank holds rows of B"
        assert eng.gatv2_built() is False
        for ndt in (np.float64, np.float32):
            V, Vd, Bd = data[ndt]["V"], data[ndt]["Vd"], data[ndt]["Bd"]
            tdt = Vd.dtype
            C0 = nan(tdt, e0 - s0, n)
            eng.exec(0, Bd[b0:b1], C0)
            torch.cuda.synchronize()
            for H in (1, 3):
                xtd, avd = data[ndt][H]
                vec = (lambda t: t.view(-1)) if H == 1 else (lambda t: t)         # one head: the per-row arrays are 1-D
                for bias in (False, True):
                    full = fulls[ndt, H, bias]
                    what = (me, layout, ndt.__name__, H, bias)

                    def check(O, lse, p, tag):
                        assert torch.equal(O, full["O"][s0:e0]), (what, tag, "O")
                        assert torch.equal(lse.view(-1, H), full["lse"][s0:e0]), (what, tag, "lse")
                        assert torch.equal(p.view(-1, H), full["p"][lo:hi]), (what, tag, "p_out")
                    for timing in (True, False, False):
                        eng.set_timing(timing)
                        O, lse, p = nan(tdt, e0 - s0, n), nan(tdt, e0 - s0, H), nan(tdt, hi - lo, H)
                        eng.gatv2_attention(0, xtd[s0:e0], avd, Vd[b0:b1], O, slope=slope, bias=bias, lse=vec(lse), p_out=vec(p), heads=H)
                        torch.cuda.synchronize()
                        assert eng.gatv2_built() is True, what                # also on a rank without rows
                        check(O, lse, p, "timing %s" % timing)
                    if bias and H == 3 and layout == "balanced":
                        # column-major XS and O on the device; host XS, O, lse and p_out in both layouts
                        Ocm = nan(tdt, n, e0 - s0)
                        eng.gatv2_attention(1, xtd[s0:e0], avd, Vd[b0:b1].t().contiguous(), Ocm, slope=slope, bias=bias, heads=H)
                        torch.cuda.synchronize()
                        assert torch.equal(Ocm.t(), full["O"][s0:e0]), (what, "layout 1 on the device")
                        for lay in (0, 1):
                            Vh = np.ascontiguousarray(V[b0:b1] if lay == 0 else V[b0:b1].T)
                            Oh = np.full((e0 - s0, n) if lay == 0 else (n, e0 - s0), np.nan, ndt)
                            lh, ph = np.full((e0 - s0, H), np.nan, ndt), np.full((hi - lo, H), np.nan, ndt)
                            eng.gatv2_attention(lay, xtd[s0:e0], avd, Vh, Oh, slope=slope, bias=bias, lse=lh, p_out=ph, heads=H)
                            check(T(Oh if lay == 0 else Oh.T), T(lh), T(ph), "host operands, layout %d" % lay)
            C1 = nan(tdt, e0 - s0, n)
            eng.exec(0, Bd[b0:b1], C1)
            torch.cuda.synchronize()
            assert torch.equal(C0, C1) and bool(C0.isfinite().all()), (me, layout, ndt.__name__, "an exec before and after")
            # the call on a non-blocking side stream (timing off): the default stream's bits
            eng.set_timing(False)
            xtd, avd = data[ndt][3]
            full = fulls[ndt, 3, True]
            O, lse, p = nan(tdt, e0 - s0, n), nan(tdt, e0 - s0, 3), nan(tdt, hi - lo, 3)
            torch.cuda.synchronize()
            with torch.cuda.stream(S):
                eng.gatv2_attention(0, xtd[s0:e0], avd, Vd[b0:b1], O, slope=slope, bias=True, lse=lse, p_out=p, heads=3)
            S.synchronize()
            torch.cuda.synchronize()
            for got, want in ((O, full["O"][s0:e0]), (lse, full["lse"][s0:e0]), (p, full["p"][lo:hi])):
                assert np.array_equal(bits(got), bits(want)), (me, layout, ndt.__name__, "the side stream's result differs")
        eng.free()
        dist.barrier()
    torch.cuda.synchronize()
    lib.crp_stream_destroy(sp)
    A.free()
    if me == 0:
        print("GPU_DIST_GATV2_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
