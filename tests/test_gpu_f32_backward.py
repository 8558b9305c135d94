"""GPU: the fp32 transposed product and the device-resident value updates.  crp_scatter_add_rows_f32 and crp_gather_vals_*
directly, bit for bit against numpy; exec_t_f32 of the row-parallel engine at one rank against the entrywise fp32 bound
(tests/fp32_ref.py) on the numpy transpose and, bit for bit, against the product on a transposed handle; update_values_dev
against a twin engine updated from the host, bit for bit in every product that reads the values; the step sddmm ->
update_values_dev -> exec -> exec_t_f32 on the device against the same step through the host; 2 and 4 ranks sharing the GPU
(tests/gpu_dist_f32_backward_worker.py, tests/gpu_dist_para2d_f32_backward_worker.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fp32_ref
from conftest import FP64_TOL, ROOT
from test_transpose import numpy_transpose

pytestmark = pytest.mark.gpu


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _mantissa_full(rng, shape, dt):
    """values with full mantissas over scales 2^-20 .. 2^20: the order of the additions shows in the last bits"""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, size=shape))).astype(dt)


def test_scatter_add_rows_f32_adds_in_list_order(crp, gpu):
    """crp_scatter_add_rows_f32: dst[row] += the listed source rows, one fp32 addition after the other; the segment list of
    test_gpu_transpose.py::test_scatter_add_rows_adds_in_list_order (an empty segment, a repeated source row); n = 24 with
    ldd = 24 runs the 16-byte instance, everything else the element instance.  Columns past n are not touched."""
    import torch
    lib = crp.load()
    rng = np.random.default_rng(4)
    rows = np.array([3, 0, 17, 29], np.int32)
    ptr = np.array([0, 3, 4, 4, 9], np.int32)
    pos = np.array([5, 2, 39, 7, 1, 1, 8, 30, 0], np.int32)
    d_rows, d_ptr, d_pos = _dev(gpu, rows, ptr, pos)
    for n in (24, 30, 7):
        for ldd in (n, n + 1):
            src = _mantissa_full(rng, (40, n), np.float32)
            dst = _mantissa_full(rng, (30, ldd), np.float32)
            want = dst.copy()
            for t, r in enumerate(rows):
                for k in range(ptr[t], ptr[t + 1]):
                    want[r, :n] = want[r, :n] + src[pos[k]]
            assert want.dtype == np.float32
            d_src, d_dst = _dev(gpu, src, dst)
            assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
            rc = lib.crp_scatter_add_rows_f32(rows.size, n, d_rows.data_ptr(), d_ptr.data_ptr(), d_pos.data_ptr(), d_src.data_ptr(), n,
                                              d_dst.data_ptr(), ldd, None)
            torch.cuda.synchronize()
            assert rc == 0 and np.array_equal(d_dst.cpu().numpy(), want), (n, ldd)


def test_gather_vals_widens_and_gathers_exactly(crp, gpu):
    """crp_gather_vals_f64 / _f32_f64: dst[i] = (double) src[map ? map[i] : i], 10 007 entries, a map with repeats."""
    import torch
    lib = crp.load()
    rng = np.random.default_rng(9)
    nn, POISON = 10007, 777.0
    idx = rng.integers(0, nn, size=nn).astype(np.int32)
    idx[:50] = idx[50]                                                   # one position fifty times
    assert np.unique(idx).size < nn
    d_idx, = _dev(gpu, idx)
    for dt, fn in ((np.float64, lib.crp_gather_vals_f64), (np.float32, lib.crp_gather_vals_f32_f64)):
        src = _mantissa_full(rng, nn, dt)
        d_src, = _dev(gpu, src)
        for mp, want in ((None, src.astype(np.float64)), (d_idx.data_ptr(), src[idx].astype(np.float64))):
            d_dst = torch.full((nn + 3,), POISON, dtype=torch.float64, device=gpu)
            rc = fn(nn, mp, d_src.data_ptr(), d_dst.data_ptr(), None)
            torch.cuda.synchronize()
            got = d_dst.cpu().numpy()
            assert rc == 0 and np.array_equal(got[:nn], want) and (got[nn:] == POISON).all(), (dt.__name__, mp is None)


def _matrices():
    """rectangular with empty columns met by no row, and banded with A != A^T; values by the data rule of fp32_ref"""
    from crp_spmm_amd import gen
    rng = np.random.default_rng(21)
    rp, ci, va = gen.random_csr(3000, 1700, 40)
    yield "random_csr", rp, ci, fp32_ref.data_values(rng, va.size), 1700
    rp, ci, va = gen.banded_fem(6000, offsets=(1, 2, 3, 4, 50, 51, 1400))
    yield "banded_fem", rp, ci, fp32_ref.data_values(rng, va.size), 6000


def _run(gpu, call, shape, tdt):
    import torch
    out = torch.full(shape, float("nan"), dtype=tdt, device=gpu)
    call(out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


@pytest.mark.parametrize("n", [7, 48, 256])
def test_exec_t_f32_at_one_rank(crp, orc, gpu, n):
    """n = 7: an ld32 pad and the element accumulate; 48 and 256: the half-piece and the one-piece team instance."""
    import torch
    from crp_spmm_amd import comm, engine, hip
    sc = comm.SelfComm()
    rng = np.random.default_rng(100 + n)
    for name, rp, ci, va, k in _matrices():
        m = rp.size - 1
        rp_t, ci_t, va_t, _ = numpy_transpose(rp, ci, va, k)
        Y32, B32 = fp32_ref.data_B(rng, (m, n)), fp32_ref.data_B(rng, (k, n))
        rb = fp32_ref.f32_bound(rp_t, ci_t, va_t, Y32)
        e = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
        Yd, Bd = _dev(gpu, Y32, B32)
        _run(gpu, lambda o: e.exec(0, Bd, o), (m, n), torch.float32)
        assert not e.transposed_built, (name, n)
        got = _run(gpu, lambda o: e.exec_t_f32(0, Yd, o), (k, n), torch.float32)
        assert e.transposed_built, (name, n)
        fp32_ref.check_f32_bound(rp_t, ci_t, va_t, Y32, got, what="%s n=%d exec_t_f32" % (name, n), ref_bound=rb)
        assert np.array_equal(got, _run(gpu, lambda o: e.exec_t_f32(0, Yd, o), (k, n), torch.float32)), (name, n, "repeat")
        if n % 4 == 0:
            At = hip.CsrDev.from_transpose(m, k, rp, ci, va)
            for variant in (0, 1, 5):
                e.set_variant_f32(variant)
                eng = _run(gpu, lambda o: e.exec_t_f32(0, Yd, o), (k, n), torch.float32)
                han = _run(gpu, lambda o: hip.spmm_csr_f32(At, Yd, o, n=n, variant=variant), (k, n), torch.float32)
                assert np.array_equal(eng, han), (name, n, variant, "engine against the transposed handle")
                fp32_ref.check_f32_bound(rp_t, ci_t, va_t, Y32, eng, what="%s n=%d variant %d" % (name, n, variant), ref_bound=rb)
            e.set_variant_f32(0)
            At.free()
        # host operands, column-major
        Ch = np.full((n, k), np.nan, np.float32)
        e.exec_t_f32(1, np.ascontiguousarray(Y32.T), Ch)
        fp32_ref.check_f32_bound(rp_t, ci_t, va_t, Y32, Ch.T, what="%s n=%d host cm" % (name, n), ref_bound=rb)
        # the fp64 form on the same engine
        Y64 = Y32.astype(np.float64)
        c64 = _run(gpu, lambda o: e.exec_t(0, _dev(gpu, Y64)[0], o), (k, n), torch.float64)
        assert orc.rel_fro_err(rb[0], c64) <= FP64_TOL, (name, n, "fp64 exec_t")
        # twice the values: every product, partial sum and rounding doubles exactly
        e.update_values(2.0 * va)
        twice = _run(gpu, lambda o: e.exec_t_f32(0, Yd, o), (k, n), torch.float32)
        assert np.abs(got).max() > 0 and np.array_equal(twice, 2 * got), (name, n, "update_values(2 va)")
        e.free()
    sc.free()


def _five(gpu, e, ops, m, k, n, nnz):
    """the five products that read A's values: exec, exec on float32, exec_t, exec_t_f32, sddmm(mode=1) (both dtypes)"""
    import torch
    B64, B32, Y64, Y32 = ops
    return [_run(gpu, lambda o: e.exec(0, B64, o), (m, n), torch.float64),
            _run(gpu, lambda o: e.exec(0, B32, o), (m, n), torch.float32),
            _run(gpu, lambda o: e.exec_t(0, Y64, o), (k, n), torch.float64),
            _run(gpu, lambda o: e.exec_t_f32(0, Y32, o), (k, n), torch.float32),
            _run(gpu, lambda o: e.sddmm(0, Y64, B64, o, mode=1), (nnz,), torch.float64),
            _run(gpu, lambda o: e.sddmm(0, Y32, B32, o, mode=1), (nnz,), torch.float32)]


@pytest.mark.parametrize("n", [7, 48])
def test_update_values_dev_equals_the_host_update_bit_for_bit(crp, gpu, n):
    import torch
    from crp_spmm_amd import comm, engine
    name, rp, ci, va, k = list(_matrices())[0]
    m, nnz = rp.size - 1, ci.size
    rng = np.random.default_rng(5 + n)
    sc = comm.SelfComm()
    ea = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
    eb = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
    assert ea.overlap_rows() == (0, 0)
    B32, Y32 = fp32_ref.data_B(rng, (k, n)), fp32_ref.data_B(rng, (m, n))
    ops = _dev(gpu, B32.astype(np.float64), B32, Y32.astype(np.float64), Y32)
    # the formats exist with the old values before the first update
    old = [_run(gpu, lambda o: e.exec(0, ops[0], o), (m, n), torch.float64) for e in (ea, eb)]
    assert np.array_equal(*old)
    _run(gpu, lambda o: ea.exec(0, ops[1], o), (m, n), torch.float32)
    assert not ea.host_values_stale

    # ---- fp64 values, before the first exec_t: the transposed matrices built afterwards see them
    v2 = fp32_ref.data_values(rng, nnz)
    ea.update_values_dev(_dev(gpu, v2)[0])
    eb.update_values(v2)
    assert ea.host_values_stale and not eb.host_values_stale and not ea.transposed_built
    new = _run(gpu, lambda o: ea.exec(0, ops[0], o), (m, n), torch.float64)
    assert not np.array_equal(new, old[0])
    assert ea.host_values_stale
    for tag, a, b in zip(("exec", "exec f32", "exec_t", "exec_t_f32", "sddmm", "sddmm f32"), _five(gpu, ea, ops, m, k, n, nnz),
                         _five(gpu, eb, ops, m, k, n, nnz)):
        assert np.array_equal(a, b), (n, tag, "fp64 values, transposed matrices built after the update")
    assert ea.transposed_built and eb.transposed_built

    # ---- fp64 values again, the transposed matrices exist; the host mirror follows when it is read
    v3 = fp32_ref.data_values(rng, nnz)
    ea.update_values_dev(_dev(gpu, v3)[0])
    eb.update_values(v3)
    assert ea.host_values_stale
    for tag, a, b in zip(("exec", "exec f32", "exec_t", "exec_t_f32", "sddmm", "sddmm f32"), _five(gpu, ea, ops, m, k, n, nnz),
                         _five(gpu, eb, ops, m, k, n, nnz)):
        assert np.array_equal(a, b), (n, tag, "fp64 values")
    assert ea.host_values_stale
    assert np.array_equal(ea.plan()["A_val"], v3) and not ea.host_values_stale

    # ---- fp32 values: equal to the host update with the widened values
    v4 = fp32_ref.data_values(rng, nnz).astype(np.float32)
    ea.update_values_dev(_dev(gpu, v4)[0])
    eb.update_values(v4.astype(np.float64))
    for tag, a, b in zip(("exec", "exec f32", "exec_t", "exec_t_f32", "sddmm", "sddmm f32"), _five(gpu, ea, ops, m, k, n, nnz),
                         _five(gpu, eb, ops, m, k, n, nnz)):
        assert np.array_equal(a, b), (n, tag, "fp32 values")
    assert np.array_equal(ea.plan()["A_val"], v4.astype(np.float64))
    # a host update afterwards wins and clears the flag
    ea.update_values_dev(_dev(gpu, v3)[0])
    ea.update_values(v2)
    assert not ea.host_values_stale and np.array_equal(ea.plan()["A_val"], v2)
    eb.update_values(v2)
    assert np.array_equal(_run(gpu, lambda o: ea.exec_t_f32(0, ops[3], o), (k, n), torch.float32),
                          _run(gpu, lambda o: eb.exec_t_f32(0, ops[3], o), (k, n), torch.float32))
    with pytest.raises(ValueError):
        ea.update_values_dev(_dev(gpu, v2[:-1])[0])
    ea.free()
    eb.free()
    sc.free()


def test_one_step_on_the_device_equals_the_step_through_the_host(crp, gpu):
    """sddmm (float32, mode 0) -> new values -> exec -> exec_t_f32: with `out` on the device and update_values_dev nothing is
    copied to the host between the calls; the twin engine takes `out` to the host, widens it there and updates from the host."""
    import torch
    from crp_spmm_amd import comm, engine
    name, rp, ci, va, k = list(_matrices())[1]
    m, nnz, n = rp.size - 1, ci.size, 48
    rng = np.random.default_rng(77)
    sc = comm.SelfComm()
    ea = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
    eb = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
    X, Y, B, G = (fp32_ref.data_B(rng, s) for s in ((m, n), (k, n), (k, n), (m, n)))
    Xd, Yd, Bd, Gd = _dev(gpu, X, Y, B, G)
    Ca = torch.full((m, n), float("nan"), dtype=torch.float32, device=gpu)
    Ga = torch.full((k, n), float("nan"), dtype=torch.float32, device=gpu)
    out = torch.full((nnz,), float("nan"), dtype=torch.float32, device=gpu)
    ea.set_timing(False)
    for _step in range(2):
        ea.sddmm(0, Xd, Yd, out)
        ea.update_values_dev(out)
        ea.exec(0, Bd, Ca)
        ea.exec_t_f32(0, Gd, Ga)
    torch.cuda.synchronize()
    assert ea.host_values_stale
    Cb = torch.full((m, n), float("nan"), dtype=torch.float32, device=gpu)
    Gb = torch.full((k, n), float("nan"), dtype=torch.float32, device=gpu)
    oh = np.full(nnz, np.nan, np.float32)
    for _step in range(2):
        eb.sddmm(0, Xd, Yd, oh)
        eb.update_values(oh.astype(np.float64))
        eb.exec(0, Bd, Cb)
        eb.exec_t_f32(0, Gd, Gb)
    torch.cuda.synchronize()
    ca, ga = Ca.cpu().numpy(), Ga.cpu().numpy()
    assert not np.isnan(ca).any() and not np.isnan(ga).any() and np.abs(ga).max() > 0
    assert np.array_equal(out.cpu().numpy(), oh)
    assert np.array_equal(ca, Cb.cpu().numpy()) and np.array_equal(ga, Gb.cpu().numpy())
    assert np.array_equal(ea.plan()["A_val"], oh.astype(np.float64))
    ea.free()
    eb.free()
    sc.free()


def _worker(script, ok, world, port, native, extra=None):
    env = dict(os.environ)
    env.update(extra or {})
    env["OMP_NUM_THREADS"] = "1"
    if native:
        env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        env["CRPSPMM_EXPECT_NATIVE_RCCL"] = "1"
        env.pop("CRPSPMM_EXCHANGE", None)
    else:
        env["CRPSPMM_EXCHANGE"] = "host"
        env.pop("CRPSPMM_EXPECT_NATIVE_RCCL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", script)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%s world=%d" % (ok, world) in r.stdout


WORKERS = {"rp": ("gpu_dist_f32_backward_worker.py", "GPU_DIST_F32_BACKWARD_WORKER_OK", 29960),
           "para2d": ("gpu_dist_para2d_f32_backward_worker.py", "GPU_DIST_PARA2D_F32_BACKWARD_WORKER_OK", 29980)}


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("which", sorted(WORKERS))
def test_multi_rank_one_gpu(which, world):
    script, ok, port = WORKERS[which]
    _worker(script, ok, world, port + world, native=False)


def test_para2d_update_values_dev_without_a_device_all_gather():
    """CRPSPMM_REPLICATE=host: the grid row's slices go through allgatherv_bytes on host copies (the path of a communicator
    without allgatherv_dev); the short form of the 2D worker, 2 ranks."""
    script, ok, port = WORKERS["para2d"]
    _worker(script, ok, 2, port + 7, native=False, extra={"CRPSPMM_REPLICATE": "host", "CRP_TEST_HOST_GATHER": "1"})


def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("which", sorted(WORKERS))
def test_native_rccl_multi_gpu(which, world):
    """The same workers with one rank per GPU and the native RCCL exchange; skipped on a box with fewer GPUs, as
    tests/test_gpu_transpose.py::test_exec_t_native_rccl_multi_gpu is."""
    if _gpu_count() < world:
        pytest.skip("needs %d GPUs (native RCCL refuses two ranks on one device)" % world)
    script, ok, port = WORKERS[which]
    _worker(script, ok, world, port + 10 + world, native=True)
