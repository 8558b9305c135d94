"""Worker for tests/test_gpu_f32_backward.py: the row-parallel engine's fp32 transposed product and its device-resident value
updates on N ranks -- sharing ONE GPU with device payloads staged through the host (the rehearsal mode of
tests/gpu_dist_t_worker.py), or with a GPU per rank and the native RCCL exchange.  Every rank's rows of C := A^T * B meet the
entrywise fp32 bound of tests/fp32_ref.py against the GLOBAL transpose, whatever the cut into ranks, and so do its rows of the
forward product the later checks compare with; a twin engine updated from
the host gives the same bits as the one updated from device memory, split into interior and boundary rows or not."""
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
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def run(call, shape, tdt):
        out = torch.full(shape, float("nan"), dtype=tdt, device=dev)
        call(out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert not np.isnan(got).any()
        return got

    m = k = 6000
    rng = np.random.default_rng(31)                                   # the same stream on every rank
    rp_b, ci_b, va_b = gen.banded_fem(m, offsets=(1, 2, 3, 4, 50, 51, 1400), seed=5)
    rp_r, ci_r, va_r = gen.random_csr(m, k, 30)
    mats = (("banded_fem", (rp_b, ci_b, fp32_ref.data_values(rng, va_b.size))),           # A != A^T: independent values
            ("random_csr", (rp_r, ci_r, fp32_ref.data_values(rng, va_r.size))))
    for name, (rp, ci, va) in mats:
        rp_t, ci_t, va_t = np_transpose(rp, ci, va, k)
        rb = planner.csr_mat_row_partition(rp, P)
        s, e = int(rb[me]), int(rb[me + 1])
        mine = slice(int(rp[s]), int(rp[e]))
        nnz = mine.stop - mine.start
        for n in (7, 256):
            Y32, B32 = fp32_ref.data_B(rng, (m, n)), fp32_ref.data_B(rng, (k, n))
            ref, bound = fp32_ref.f32_bound(rp_t, ci_t, va_t, Y32)
            ref_f, bound_f = fp32_ref.f32_bound(rp, ci, va, B32)                  # the forward product, global as well
            mk = lambda: engine.RpSpmm(s, e - s, rp[s:e + 1], ci[mine], va[mine], rb, n, world)
            eng = mk()
            if P == 2 and name == "banded_fem":      # (every row of random_csr has a column of the peer's: that engine stays whole)
                assert min(eng.overlap_rows()) > 0, (me, name, n, "the overlap split should exist at P = 2")
            Yd, Bd = T(Y32[s:e]), T(B32[s:e])
            tag = (me, name, n)
            # ---- lazy build: a forward fp32 exec builds nothing transposed
            fwd = run(lambda o: eng.exec(0, Bd, o), (e - s, n), torch.float32)
            assert not eng.transposed_built, tag
            fp32_ref.check_f32_bound(rp[s:e + 1], None, None, None, fwd, what="rank %d %s n=%d forward exec" % tag,
                                     ref_bound=(ref_f[s:e], bound_f[s:e]))
            # ---- the bound, timing on: peers' part, exchange, local part, accumulate in sequence
            seq = run(lambda o: eng.exec_t_f32(0, Yd, o), (e - s, n), torch.float32)
            assert eng.transposed_built, tag
            fp32_ref.check_f32_bound(rp_t[s:e + 1], None, None, None, seq, what="rank %d %s n=%d exec_t_f32" % tag,
                                     ref_bound=(ref[s:e], bound[s:e]))
            # ---- timing off (the exchange beside the local product): no sum may change
            eng.set_timing(False)
            for rep in range(3):
                got = run(lambda o: eng.exec_t_f32(0, Yd, o), (e - s, n), torch.float32)
                assert np.array_equal(got, seq), tag + (rep, "timing off differs from timing on")
            # ---- forward unchanged: the fp32 exchange buffers are shared
            assert np.array_equal(run(lambda o: eng.exec(0, Bd, o), (e - s, n), torch.float32), fwd), tag + ("forward after exec_t_f32",)
            # ---- the fp64 form on the same engine, and host operands column-major
            eng.set_timing(True)
            c64 = run(lambda o: eng.exec_t(0, T(Y32[s:e].astype(np.float64)), o), (e - s, n), torch.float64)
            err = np.linalg.norm(c64 - ref[s:e]) / max(np.linalg.norm(ref[s:e]), 1e-300)
            assert err <= 1e-12, tag + ("fp64 exec_t", err)
            Ch = np.full((n, e - s), np.nan, np.float32)
            eng.exec_t_f32(1, np.ascontiguousarray(Y32[s:e].T), Ch)
            fp32_ref.check_f32_bound(rp_t[s:e + 1], None, None, None, Ch.T, what="rank %d %s n=%d host operands, layout 1" % tag,
                                     ref_bound=(ref[s:e], bound[s:e]))

            # ---- device value updates against a twin engine updated from the host
            twin = mk()
            Y64, B64 = T(Y32[s:e].astype(np.float64)), T(B32[s:e].astype(np.float64))

            def products(g):
                return [("exec", run(lambda o: g.exec(0, B64, o), (e - s, n), torch.float64)),
                        ("exec_t", run(lambda o: g.exec_t(0, Y64, o), (e - s, n), torch.float64)),
                        ("exec_t_f32", run(lambda o: g.exec_t_f32(0, Yd, o), (e - s, n), torch.float32)),
                        ("sddmm", run(lambda o: g.sddmm(0, Y64, B64, o, mode=1), (nnz,), torch.float64))]

            for timing in (True, False):
                eng.set_timing(timing)
                twin.set_timing(timing)
                v = fp32_ref.data_values(rng, va.size)[mine]
                eng.update_values_dev(T(v))           # (the engine's transposed matrices exist, the twin's are built from the host values)
                twin.update_values(v)
                assert eng.host_values_stale and not twin.host_values_stale, tag
                for (what, a), (_w, b) in zip(products(eng), products(twin)):
                    assert np.array_equal(a, b), tag + (timing, what, "update_values_dev differs from update_values")
                v32 = fp32_ref.data_values(rng, va.size)[mine].astype(np.float32)
                eng.update_values_dev(T(v32))
                twin.update_values(v32.astype(np.float64))
                for (what, a), (_w, b) in zip(products(eng), products(twin)):
                    assert np.array_equal(a, b), tag + (timing, what, "fp32 values")
            assert eng.host_values_stale
            assert np.array_equal(eng.plan()["A_val"], v32.astype(np.float64)) and not eng.host_values_stale, tag
            eng.free()
            twin.free()
            dist.barrier()
    if me == 0:
        print("GPU_DIST_F32_BACKWARD_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
