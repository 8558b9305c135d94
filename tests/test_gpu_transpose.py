"""GPU: C := A^T * B.  The device path of crp_csr_transpose (csrc/transpose_kernels.hip) against the host path, bit for
bit, over every tier of output-row length; bad inputs on the device; products, value updates and the fp32 path on
transposed handles (crp_csr_dev_create_t); the row-parallel engine's exec_t at one rank (adjoint identity) and at 2 and 4
ranks sharing the GPU (tests/gpu_dist_t_worker.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import FP64_TOL, ROOT
from test_transpose import numpy_transpose

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-5      # the existing fp32 bound: fp32 path against the fp64 oracle, relative Frobenius error


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _tier_columns(seed=1):
    """a 75 000 x 3000 matrix whose COLUMN counts sit on every tier edge of the device sort (the edge list of _tier_matrix in
    tests/test_gpu_graph_part.py: 0, 1, 2, 63 .. 66, 127 .. 129, the LDS limit -1 / +0 / +1, 70 000, 70 001 -- two columns
    are dense) plus random ones; the entries of a column come from distinct rows, met in unsorted column order"""
    from crp_spmm_amd import partition
    rng = np.random.default_rng(seed)
    nrow, ncol = 75000, 3000
    cnt = rng.integers(0, 120, ncol)
    edges = [0, 1, 2, 63, 64, 65, 66, 127, 128, 129, partition.PERMUTE_LDS_PAIRS - 1, partition.PERMUTE_LDS_PAIRS,
             partition.PERMUTE_LDS_PAIRS + 1, 70000, 70001]
    pos = rng.choice(ncol, size=len(edges), replace=False)
    cnt[pos] = edges
    rows = np.concatenate([rng.choice(nrow, size=c, replace=False) for c in cnt]).astype(np.int64)
    cols = np.repeat(np.arange(ncol), cnt)
    # a few duplicate (row, column) pairs: the tie rule
    dup = np.flatnonzero(~np.isin(cols, pos))[:500]        # (not in the columns whose counts sit on an edge)
    rows = np.concatenate([rows, rows[dup]])
    cols = np.concatenate([cols, cols[dup]])
    shuffle = rng.permutation(rows.size)                   # unsorted columns inside the rows
    rows, cols = rows[shuffle], cols[shuffle]
    order = np.argsort(rows, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrow))]).astype(np.int32)
    return rp, cols[order].astype(np.int32), rng.standard_normal(rows.size), ncol


def _host_and_device(gpu, rp, ci, va, ncol):
    import torch
    from crp_spmm_amd import hip
    want = hip.csr_transpose(rp, ci, va, ncol)
    got = hip.csr_transpose(*_dev(gpu, np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float64)), ncol)
    torch.cuda.synchronize()
    return want, [t.cpu().numpy() for t in got]


def _assert_same(want, got, tag):
    for what, w, g in zip(("rowptr_t", "colidx_t", "val_t", "tmap"), want, got):
        assert w.dtype == g.dtype and w.shape == g.shape and np.array_equal(w, g), (tag, what)


def test_device_transpose_matches_host_on_every_tier(crp, gpu):
    rp, ci, va, ncol = _tier_columns()
    counts = np.bincount(ci, minlength=ncol)
    from crp_spmm_amd import partition
    L = partition.PERMUTE_LDS_PAIRS
    assert {0, 1, 63, 64, 65, 66, L - 1, L, L + 1, 70000, 70001} <= set(counts.tolist())
    want, got = _host_and_device(gpu, rp, ci, va, ncol)
    _assert_same(want, got, "tiers")
    _assert_same(numpy_transpose(rp, ci, va, ncol), got, "tiers against numpy")


def test_device_transpose_matches_host_on_stencil_matrices(crp, gpu):
    from crp_spmm_amd import gen
    for name, (rp, ci, va) in (("kkt3d(10)", gen.kkt3d(10)), ("fem3d(7)", gen.fem3d(7))):
        want, got = _host_and_device(gpu, rp, ci, va, rp.size - 1)
        _assert_same(want, got, name)
    # rectangular, with empty rows, and the degenerate shapes
    rp, ci, va = gen.random_csr(3000, 1700, 40, empty_every=13)
    _assert_same(*_host_and_device(gpu, rp, ci, va, 1700), "random_csr")
    for nrow, ncol in ((0, 7), (5, 0), (4, 3)):
        _assert_same(*_host_and_device(gpu, np.zeros(nrow + 1, np.int32), np.zeros(0, np.int32), np.zeros(0), ncol), (nrow, ncol))


def test_device_transpose_refuses_bad_input(crp, gpu):
    import torch
    from crp_spmm_amd import _lib, gen, hip
    lib = _lib.load()
    rp, ci, va = gen.random_csr(500, 300, 30, seed=3)
    ncol, nnz = 300, ci.size
    SENT = -77

    def run(rp_, ci_, host_out=False, null_out=False):
        d_rp, d_ci, d_va = _dev(gpu, rp_, ci_, va)
        rp_t = torch.full((ncol + 1,), SENT, dtype=torch.int32, device=gpu)
        ci_t = torch.full((nnz,), SENT, dtype=torch.int32, device=gpu)
        va_t = torch.full((nnz,), float(SENT), dtype=torch.float64, device=gpu)
        tmap = torch.full((nnz,), SENT, dtype=torch.int32, device=gpu)
        h_ci_t = np.full(nnz, SENT, np.int32)
        rc = lib.crp_csr_transpose(rp.size - 1, ncol, C.c_void_p(d_rp.data_ptr()), C.c_void_p(d_ci.data_ptr()), C.c_void_p(d_va.data_ptr()),
                                   None if null_out else C.c_void_p(rp_t.data_ptr()),
                                   C.c_void_p(h_ci_t.ctypes.data) if host_out else C.c_void_p(ci_t.data_ptr()),
                                   C.c_void_p(va_t.data_ptr()), C.c_void_p(tmap.data_ptr()), None)
        torch.cuda.synchronize()
        untouched = bool((ci_t == SENT).all()) and bool((va_t == SENT).all()) and bool((tmap == SENT).all()) and (h_ci_t == SENT).all()
        return rc, untouched

    def valid_still_matches():
        _assert_same(*_host_and_device(gpu, rp, ci, va, ncol), "after an error")

    bad = ci.copy()
    bad[nnz // 2] = ~5
    assert run(rp, bad) == (hip.T_ECOL, True)
    valid_still_matches()
    bad = ci.copy()
    bad[7] = ncol
    assert run(rp, bad) == (hip.T_ECOL, True)
    valid_still_matches()
    bad = rp.copy()
    bad[0] = 1
    assert run(bad, ci) == (hip.T_EPTR, True)
    valid_still_matches()
    bad = rp.copy()
    bad[200] = bad[199] - 1
    assert run(bad, ci) == (hip.T_EPTR, True)
    valid_still_matches()
    assert run(rp, ci, null_out=True) == (hip.T_EARG, True)
    valid_still_matches()
    assert run(rp, ci, host_out=True) == (hip.T_EMIXED, True)
    valid_still_matches()
    with pytest.raises(hip.TransposeError) as ei:
        hip.csr_transpose(_dev(gpu, rp)[0], ci, va, ncol)                # device rowptr, host colidx
    assert ei.value.code == hip.T_EMIXED
    # the handle constructor passes the same codes on
    bad = ci.copy()
    bad[3] = -1
    with pytest.raises(hip.TransposeError) as ei:
        hip.CsrDev.from_transpose(rp.size - 1, ncol, rp, bad, va)
    assert ei.value.code == hip.T_ECOL


def _product_matrices():
    from crp_spmm_amd import gen
    rp, ci, va = gen.random_csr(3000, 1700, 40)
    yield "random_csr", rp, ci, va, 1700
    rp, ci, va = gen.kkt3d(9)
    yield "kkt3d(9)", rp, ci, va, rp.size - 1
    rp, ci, va = gen.banded_fem(6000, offsets=(1, 2, 3, 4, 50, 51, 1400))
    va = va * (1.0 + 0.37 * np.sin(np.arange(va.size)))                     # A != A^T
    yield "banded_fem", rp, ci, va, 6000


def test_product_on_a_transposed_handle(crp, orc, gpu):
    """spmm_csr on CsrDev.from_transpose equals, bit for bit, spmm_csr on a handle created from the numpy-transposed arrays
    (the same CSR, so the same formats and kernel), resolves to the same variant, and meets the oracle at the fp64 bound."""
    import torch
    from crp_spmm_amd import hip
    for name, rp, ci, va, ncol in _product_matrices():
        nrow = rp.size - 1
        rp_t, ci_t, va_t, _ = numpy_transpose(rp, ci, va, ncol)
        At = hip.CsrDev.from_transpose(nrow, ncol, rp, ci, va)
        Ar = hip.CsrDev(ncol, nrow, rp_t, ci_t, va_t)
        assert At.is_transposed and not Ar.is_transposed
        assert At.nrow == ncol and At.nnz == Ar.nnz == ci.size
        assert crp.load().crp_csr_dev_nrow(At.handle) == ncol
        for n in (8, 24, 32, 64, 96, 256):
            B = orc.fill_B(0, nrow, 0, n)
            Bd = torch.from_numpy(B).to(gpu)
            Ct = torch.full((ncol, n), float("nan"), dtype=torch.float64, device=gpu)
            Cr = torch.full((ncol, n), float("nan"), dtype=torch.float64, device=gpu)
            hip.spmm_csr(At, Bd, Ct)
            hip.spmm_csr(Ar, Bd, Cr)
            torch.cuda.synchronize()
            assert np.array_equal(Ct.cpu().numpy(), Cr.cpu().numpy()), (name, n)
            err = orc.rel_fro_err(orc.spmm_csr(rp_t, ci_t, va_t, B), Ct.cpu().numpy())
            assert err <= FP64_TOL, (name, n, err)
            assert At.resolved_variant(n) == Ar.resolved_variant(n), (name, n)
            lib = crp.load()
            assert lib.crp_csr_dev_last_variant(At.handle) == lib.crp_csr_dev_last_variant(Ar.handle), (name, n)
        for n in (64, 128):
            B = orc.fill_B(0, nrow, 0, n)
            Bf = torch.from_numpy(B.astype(np.float32)).to(gpu)
            Cf = torch.full((ncol, n), float("nan"), dtype=torch.float32, device=gpu)
            hip.spmm_csr_f32(At, Bf, Cf)
            torch.cuda.synchronize()
            err = orc.rel_fro_err(orc.spmm_csr(rp_t, ci_t, va_t, B), Cf.cpu().numpy().astype(np.float64))
            assert err <= FP32_TOL, (name, n, err)
        At.free()
        Ar.free()


@pytest.mark.parametrize("n,variant", [(256, 5), (48, 3)])
def test_update_values_on_a_transposed_handle(crp, orc, gpu, n, variant):
    """New values come in A's order, from a host pointer and from a device pointer; the product afterwards is bit-identical
    to that of a fresh transposed handle created with those values.  The team format (n = 256) or the row-panel format
    (n = 48) exists before the update, so its slot map carries the values."""
    import torch
    from crp_spmm_amd import hip
    for name, rp, ci, va, ncol in _product_matrices():
        nrow = rp.size - 1
        B = orc.fill_B(0, nrow, 0, n)
        Bd = torch.from_numpy(B).to(gpu)
        new = 2.0 * va + 1.0
        fresh = hip.CsrDev.from_transpose(nrow, ncol, rp, ci, new)
        Cw = torch.full((ncol, n), float("nan"), dtype=torch.float64, device=gpu)
        hip.spmm_csr(fresh, Bd, Cw, variant=variant)
        torch.cuda.synchronize()
        want = Cw.cpu().numpy()
        rp_t, ci_t, va_t, _ = numpy_transpose(rp, ci, new, ncol)
        assert orc.rel_fro_err(orc.spmm_csr(rp_t, ci_t, va_t, B), want) <= FP64_TOL, (name, n)
        for source in ("host", "device"):
            At = hip.CsrDev.from_transpose(nrow, ncol, rp, ci, va)
            Cd = torch.full((ncol, n), float("nan"), dtype=torch.float64, device=gpu)
            hip.spmm_csr(At, Bd, Cd, variant=variant)                        # builds the format with the old values
            torch.cuda.synchronize()
            assert not np.array_equal(Cd.cpu().numpy(), want)
            At.update_values(new if source == "host" else torch.from_numpy(new).to(gpu))
            Cd.fill_(float("nan"))
            hip.spmm_csr(At, Bd, Cd, variant=variant)
            torch.cuda.synchronize()
            assert np.array_equal(Cd.cpu().numpy(), want), (name, n, source)
            # a format built AFTER the update sees the new values too (from the host copies, or from the device CSR)
            Cd.fill_(float("nan"))
            hip.spmm_csr(At, Bd, Cd, variant=1)
            Cw.fill_(float("nan"))
            hip.spmm_csr(fresh, Bd, Cw, variant=1)
            other = 3 if variant == 5 else 5
            C2, W2 = torch.empty_like(Cd), torch.empty_like(Cd)
            hip.spmm_csr(At, Bd, C2, variant=other)
            hip.spmm_csr(fresh, Bd, W2, variant=other)
            torch.cuda.synchronize()
            assert np.array_equal(Cd.cpu().numpy(), Cw.cpu().numpy()), (name, n, source, "csr")
            assert np.array_equal(C2.cpu().numpy(), W2.cpu().numpy()), (name, n, source, "later format")
            At.free()
        fresh.free()


def test_adjoint_identity_on_the_engine_at_one_rank(crp, orc, gpu):
    """<A B, Y> = <B, A^T Y> for C1 = exec(B), C2 = exec_t(Y), to 1e-12 * |C1| |Y|; rectangular A; lazy build; value updates."""
    import torch
    from crp_spmm_amd import comm, engine, gen
    sc = comm.SelfComm()
    for name, rp, ci, va, k in _product_matrices():
        m = rp.size - 1
        for n in (24, 256):
            e = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
            B = orc.fill_B(0, k, 0, n)
            Y = np.random.default_rng(11).standard_normal((m, n))
            Bd, Yd = _dev(gpu, B, Y)
            C1 = torch.full((m, n), float("nan"), dtype=torch.float64, device=gpu)
            C2 = torch.full((k, n), float("nan"), dtype=torch.float64, device=gpu)
            e.exec(0, Bd, C1)
            assert not e.transposed_built
            e.exec_t(0, Yd, C2)
            assert e.transposed_built
            torch.cuda.synchronize()
            c1, c2 = C1.cpu().numpy(), C2.cpu().numpy()
            lhs, rhs = float(np.vdot(c1, Y)), float(np.vdot(B, c2))
            bound = 1e-12 * np.linalg.norm(c1) * np.linalg.norm(Y)
            assert abs(lhs - rhs) <= bound, (name, n, lhs, rhs, bound)
            rp_t, ci_t, va_t, _ = numpy_transpose(rp, ci, va, k)
            ref = orc.spmm_csr(rp_t, ci_t, va_t, Y)
            assert orc.rel_fro_err(ref, c2) <= FP64_TOL, (name, n)
            # host operands, column-major
            Ch = np.full((n, k), np.nan)
            e.exec_t(1, np.ascontiguousarray(Y.T), Ch)
            assert orc.rel_fro_err(ref, Ch.T) <= FP64_TOL, (name, n, "host cm")
            e.update_values(2.0 * va)
            e.exec_t(0, Yd, C2)
            torch.cuda.synchronize()
            assert orc.rel_fro_err(2.0 * ref, C2.cpu().numpy()) <= FP64_TOL, (name, n, "update_values")
            with pytest.raises(TypeError):
                e.exec_t(0, Yd.to(torch.float32), C2.to(torch.float32))
            e.free()
    sc.free()


def test_scatter_add_rows_adds_in_list_order(crp, gpu):
    """crp_scatter_add_rows_f64: dst[row] += the listed source rows, one after the other (even and odd widths)."""
    import torch
    lib = crp.load()
    rng = np.random.default_rng(4)
    for n in (24, 7):
        src = rng.standard_normal((40, n))
        dst = rng.standard_normal((30, n + 1))
        rows = np.array([3, 0, 17, 29], np.int32)
        ptr = np.array([0, 3, 4, 4, 9], np.int32)
        pos = np.array([5, 2, 39, 7, 1, 1, 8, 30, 0], np.int32)
        want = dst.copy()
        for t, r in enumerate(rows):
            for k in range(ptr[t], ptr[t + 1]):
                want[r, :n] = want[r, :n] + src[pos[k]]
        d_src, d_dst, d_rows, d_ptr, d_pos = _dev(gpu, src, dst, rows, ptr, pos)
        rc = lib.crp_scatter_add_rows_f64(rows.size, n, d_rows.data_ptr(), d_ptr.data_ptr(), d_pos.data_ptr(), d_src.data_ptr(), n,
                                          d_dst.data_ptr(), n + 1, None)
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(d_dst.cpu().numpy(), want), n


@pytest.mark.parametrize("world", [2, 4])
def test_exec_t_multi_rank_one_gpu(world):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29840 + world), os.path.join(ROOT, "tests", "gpu_dist_t_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_T_WORKER_OK world=%d" % world in r.stdout


def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.parametrize("world", [2, 4])
def test_exec_t_native_rccl_multi_gpu(world):
    """The same worker with one rank per GPU and the native RCCL exchange; skipped on a box with fewer GPUs, as
    tests/test_gpu_dist.py::test_engines_native_rccl_multi_gpu is."""
    if _gpu_count() < world:
        pytest.skip("needs %d GPUs (native RCCL refuses two ranks on one device)" % world)
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env["CRPSPMM_EXPECT_NATIVE_RCCL"] = "1"
    env.pop("CRPSPMM_EXCHANGE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29860 + world), os.path.join(ROOT, "tests", "gpu_dist_t_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_T_WORKER_OK world=%d" % world in r.stdout
