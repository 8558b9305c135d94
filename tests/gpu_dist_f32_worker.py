"""Worker for tests/test_gpu_engine_f32.py: the fp32 exec of the 1D and 2D engines with N ranks sharing ONE GPU
(CRPSPMM_EXCHANGE=host: device payloads staged through the host and gloo, as in tests/gpu_dist_worker.py).

Checks, on every rank: accuracy against the fp64 oracle on B rounded to fp32; at fp32 variant 1 the rank's C block is
bit-identical to the one-rank fp32 variant-1 product of the whole matrix; the words handed to alltoallv_dev_f64 are
rows * round_up(n, 4) / 2 per peer; NaN and Inf in B rows that cross the exchange land exactly where the oracle has
them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_TOL = 1e-5
CALLS = []        # (send words per peer, receive words per peer) of every device all-to-all of this process


def _record_exchange(crp_comm):
    """Wrap the Python communicator's device all-to-all (before any communicator exists) to record its counts."""
    inner = crp_comm.TorchComm._alltoallv_dev_f64

    @crp_comm._fatal_on_error
    def recording(self, ctx, send, scnts, sdispls, recv, rcnts, rdispls, stream):
        P = self.nproc
        CALLS.append(([int(scnts[i]) for i in range(P)], [int(rcnts[i]) for i in range(P)]))
        return inner(self, ctx, send, scnts, sdispls, recv, rcnts, rdispls, stream)
    crp_comm.TorchComm._alltoallv_dev_f64 = recording


def _check_words(rp_eng, n, tag):
    """The last exchange carried rows * ld32 / 2 words per peer (and half the fp64 count when 4 | n)."""
    d = rp_eng.plan()
    if d["nproc"] == 1:
        assert CALLS == [], tag
        return
    assert len(CALLS) == 1, (tag, len(CALLS))
    ld32 = (n + 3) // 4 * 4
    sw, rw = CALLS[-1]
    assert sw == [int(c) // n * ld32 // 2 for c in d["rB_scnts"]], (tag, sw, list(d["rB_scnts"]))
    assert rw == [int(c) // n * ld32 // 2 for c in d["rB_rcnts"]], (tag, rw, list(d["rB_rcnts"]))
    if n % 4 == 0:
        assert sw == [int(c) // 2 for c in d["rB_scnts"]], tag


def main():
    import torch
    import torch.distributed as dist
    import oracle as orc
    from crp_spmm_amd import comm as crp_comm, engine, gen, hip, planner

    _record_exchange(crp_comm)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    crp_comm.init_process_group()
    assert crp_comm.exchange_mode() == "host"
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    m = k = 6000
    rp, ci, va = gen.banded_fem(m, offsets=(1, 2, 3, 4, 50, 51, 1400), seed=5)
    rb = planner.csr_mat_row_partition(rp, P)
    s, e = int(rb[me]), int(rb[me + 1])
    A_all = hip.CsrDev(m, k, rp, ci, va)
    for n in (24, 30, 256):
        B32 = orc.fill_B(0, k, 0, n).astype(np.float32)
        C_ref = orc.spmm_csr(rp, ci, va, B32.astype(np.float64))
        # the one-rank fp32 variant-1 product of the whole matrix
        C1d = torch.empty((m, n), dtype=torch.float32, device=dev)
        hip.spmm_csr_f32(A_all, torch.from_numpy(B32).to(dev), C1d, n=n, variant=1)
        torch.cuda.synchronize()
        C1 = C1d.cpu().numpy()

        # ---- 1D engine: device row-major, host column-major, timing on and off (the overlap split), variants 0 / 1 / 5
        eng = engine.RpSpmm(s, e - s, rp[s:e + 1], ci[rp[s]:rp[e]], va[rp[s]:rp[e]], rb, n, world)
        if P == 2:
            assert min(eng.overlap_rows()) > 0, "the overlap split should exist at P = 2"
        Bd = torch.from_numpy(B32[s:e].copy()).to(dev)
        for timing in (True, False):
            eng.set_timing(timing)
            for variant in (0, 5, 1):
                eng.set_variant_f32(variant)
                tag = (me, n, timing, variant)
                Cd = torch.full((e - s, n), float("nan"), dtype=torch.float32, device=dev)
                CALLS.clear()
                eng.exec(0, Bd, Cd)
                torch.cuda.synchronize()
                _check_words(eng, n, tag + ("1D rm",))
                got = Cd.cpu().numpy()
                assert orc.rel_fro_err(C_ref[s:e], got.astype(np.float64)) <= FP32_TOL, tag + ("1D rm",)
                if variant == 1:
                    assert np.array_equal(got.view(np.int32), C1[s:e].view(np.int32)), tag + ("1D rm bits",)
            Ch = np.full((n, e - s), np.nan, np.float32)
            eng.exec(1, np.ascontiguousarray(B32[s:e].T), Ch)                # host pointers, column-major, variant 1
            assert np.array_equal(np.ascontiguousarray(Ch.T).view(np.int32), C1[s:e].view(np.int32)), (me, n, timing, "1D cm host")
        # ---- NaN / Inf in B rows that cross the exchange (first row of rank 1, last row of rank 0, a middle row of the last rank)
        Bp = B32.copy()
        poison = [(int(rb[1]), 0, np.nan), (int(rb[1]), 3, np.inf), (int(rb[1]) - 1, 3, -np.inf), (int(rb[1]) - 1, n - 1, np.nan),
                  ((int(rb[P - 1]) + int(rb[P])) // 2, 1, np.inf)]
        for r, c, v in poison:
            Bp[r, c] = v
        with np.errstate(invalid="ignore"):
            P_ref = orc.spmm_csr(rp, ci, va, Bp.astype(np.float64))[s:e]
        Bpd = torch.from_numpy(Bp[s:e].copy()).to(dev)
        eng.set_variant_f32(1)
        for timing in (True, False):
            eng.set_timing(timing)
            Cd = torch.zeros((e - s, n), dtype=torch.float32, device=dev)
            eng.exec(0, Bpd, Cd)
            torch.cuda.synchronize()
            got = Cd.cpu().numpy().astype(np.float64)
            tag = (me, n, timing, "non-finite")
            assert np.array_equal(np.isnan(got), np.isnan(P_ref)), tag
            assert np.array_equal(np.isposinf(got), np.isposinf(P_ref)), tag
            assert np.array_equal(np.isneginf(got), np.isneginf(P_ref)), tag
            fin = np.isfinite(P_ref)
            assert orc.rel_fro_err(np.where(fin, P_ref, 0.0), np.where(fin, got, 0.0)) <= FP32_TOL, tag
        eng.print_stat()
        eng.free()
        dist.barrier()

        # ---- 2D engine on every grid of P ranks, both layouts, timing on and off
        for pn in [d for d in range(1, P + 1) if P % d == 0]:
            pm = P // pn
            ac = np.array([rb[i * pn] for i in range(pm + 1)], dtype=np.int32)
            a0 = np.zeros(P + 1, dtype=np.int32)
            for i in range(pm):
                a0[i * pn:(i + 1) * pn + 1] = planner.csr_mat_row_partition(rp[ac[i]:ac[i + 1] + 1] - rp[ac[i]], pn) + ac[i]
            bc = planner.even_displs(n, pn)
            pi, pj = me // pn, me % pn
            s0, e0 = int(a0[me]), int(a0[me + 1])
            r0, r1, c0, c1 = int(ac[pi]), int(ac[pi + 1]), int(bc[pj]), int(bc[pj + 1])
            nl = c1 - c0
            e2 = engine.Para2dSpmm(world, pm, pn, a0, ac, ac, bc, rp[s0:e0 + 1], ci[rp[s0]:rp[e0]], va[rp[s0]:rp[e0]])
            e2.rp.set_variant_f32(1)
            Bl = np.ascontiguousarray(B32[r0:r1, c0:c1])
            want = C1[r0:r1, c0:c1]
            for timing in (True, False):
                e2.rp.set_timing(timing)
                tag = (me, n, pm, pn, timing)
                Cl = torch.full((r1 - r0, nl), float("nan"), dtype=torch.float32, device=dev)
                CALLS.clear()
                e2.exec(0, torch.from_numpy(Bl).to(dev), Cl)
                torch.cuda.synchronize()
                _check_words(e2.rp, nl, tag)
                got = Cl.cpu().numpy()
                assert orc.rel_fro_err(C_ref[r0:r1, c0:c1], got.astype(np.float64)) <= FP32_TOL, tag
                assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32)), tag + ("bits",)
                Ccm = torch.full((nl, r1 - r0), float("nan"), dtype=torch.float32, device=dev)
                e2.exec(1, torch.from_numpy(np.ascontiguousarray(Bl.T)).to(dev), Ccm)
                torch.cuda.synchronize()
                assert np.array_equal(np.ascontiguousarray(Ccm.cpu().numpy().T).view(np.int32),
                                      np.ascontiguousarray(want).view(np.int32)), tag + ("cm bits",)
            e2.rp.set_variant_f32(0)
            Cl = torch.full((r1 - r0, nl), float("nan"), dtype=torch.float32, device=dev)
            e2.exec(0, torch.from_numpy(Bl).to(dev), Cl)
            torch.cuda.synchronize()
            assert orc.rel_fro_err(C_ref[r0:r1, c0:c1], Cl.cpu().numpy().astype(np.float64)) <= FP32_TOL, (me, n, pm, pn, "auto")
            e2.print_stat()
            e2.free()
            dist.barrier()
    A_all.free()
    if me == 0:
        print("GPU_DIST_F32_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
