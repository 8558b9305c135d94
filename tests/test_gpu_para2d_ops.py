"""GPU: value updates, C := A^T*B and SDDMM on the 2D engine.  crp_sum_segments_f64 / _f32 directly, bit for bit against a
left-to-right numpy sum over every size, stride and alignment at which the 16-byte and the element-wise instances run, and
its refusals; the 1 x 1 engine against the row-parallel engine on the same rows, bit for bit; every grid of 2 and 4 ranks
sharing the GPU (tests/gpu_dist_para2d_ops_worker.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _mantissa_full(rng, shape, dt):
    """values with full mantissas over scales 2^-20 .. 2^20: the order of the additions shows in the last bits"""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, size=shape))).astype(dt)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_sum_segments_adds_left_to_right_whatever_the_alignment(crp, gpu, dt):
    import torch
    lib = crp.load()
    fn = lib.crp_sum_segments_f64 if dt is np.float64 else lib.crp_sum_segments_f32
    isz = np.dtype(dt).itemsize
    rng = np.random.default_rng(11)
    POISON = 777.0
    for nseg in (1, 2, 3, 8):
        for ln in (1, 5, 258, 4099):
            for stride in (ln, ln + 3) + ((ln + 1,) if dt is np.float32 else ()):
                for off in (0, 1):                                       # src and out also one element off a 16-byte boundary
                    src = _mantissa_full(rng, off + (nseg - 1) * stride + ln + 2, dt)
                    want = src[off:off + ln].copy()
                    for j in range(1, nseg):
                        want = want + src[off + j * stride:off + j * stride + ln]
                    assert want.dtype == dt
                    d_src = torch.from_numpy(src).to(gpu)
                    d_out = torch.full((off + ln + 2,), POISON, dtype=d_src.dtype, device=gpu)
                    assert d_src.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
                    rc = fn(nseg, ln, d_src.data_ptr() + off * isz, stride, d_out.data_ptr() + off * isz, None)
                    torch.cuda.synchronize()
                    got = d_out.cpu().numpy()
                    tag = (nseg, ln, stride, off)
                    assert rc == 0, tag
                    assert np.array_equal(got[off:off + ln], want), tag
                    assert (got[:off] == POISON).all() and (got[off + ln:] == POISON).all(), tag


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_sum_segments_refusals_write_nothing(crp, gpu, dt):
    import torch
    lib = crp.load()
    fn = lib.crp_sum_segments_f64 if dt is np.float64 else lib.crp_sum_segments_f32
    d_src = torch.from_numpy(np.arange(64).astype(dt)).to(gpu)
    d_out = torch.full((16,), -3.0, dtype=d_src.dtype, device=gpu)
    s, o = d_src.data_ptr(), d_out.data_ptr()
    assert fn(2, 8, None, 8, o, None) == -1
    assert fn(2, 8, s, 8, None, None) == -1
    assert fn(0, 8, s, 8, o, None) == -1
    assert fn(-1, 8, s, 8, o, None) == -1
    assert fn(2, -1, s, 8, o, None) == -1
    assert fn(2, 8, s, 7, o, None) == -4
    assert fn(3, 8, s, 0, o, None) == -4
    assert fn(2, 0, s, 0, o, None) == 0            # nothing to do: nothing is launched
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -3.0).all()
    assert fn(1, 8, s, 0, o, None) == 0            # one segment is a copy; its stride is not read
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:8], np.arange(8).astype(dt)) and (got[8:] == -3.0).all()


M, N = 700, 23


@pytest.fixture(scope="module")
def one_rank(crp, gpu):
    """a 1 x 1 2D engine and a row-parallel engine on the same rows, with the operands both are given"""
    import torch
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.random_csr(M, M, 11, seed=5)
    sc1, sc2 = comm.SelfComm(), comm.SelfComm()
    e2 = engine.Para2dSpmm(sc2, 1, 1, [0, M], [0, M], [0, M], [0, N], rp, ci, va)
    e1 = engine.RpSpmm(0, M, rp, ci, va, [0, M], N, sc1)
    rng = np.random.default_rng(2)
    X, Y = rng.standard_normal((M, N)), rng.standard_normal((M, N))
    ops = {dt: (torch.from_numpy(X.astype(dt)).to(gpu), torch.from_numpy(Y.astype(dt)).to(gpu)) for dt in (np.float64, np.float32)}
    yield e2, e1, va, ops
    e2.free()
    e1.free()
    sc1.free()
    sc2.free()


def _run(gpu, call, shape, tdt):
    import torch
    out = torch.full(shape, float("nan"), dtype=tdt, device=gpu)
    call(out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


def test_one_rank_matches_the_row_parallel_engine_bit_for_bit(crp, gpu, one_rank):
    import torch
    e2, e1, va, ops = one_rank
    nnz = va.size
    assert e2.slice_nnz == nnz == e1.nnz() and e2.row_slice_nnz.tolist() == [nnz]
    Xd, Yd = ops[np.float64]
    C2 = _run(gpu, lambda o: e2.exec(0, Yd, o), (M, N), torch.float64)
    assert not e2.sddmm_built and not e2.rp.sddmm_built            # an exec builds nothing of the SDDMM
    assert np.array_equal(C2, _run(gpu, lambda o: e1.exec(0, Yd, o), (M, N), torch.float64))
    Ct2 = _run(gpu, lambda o: e2.exec_t(0, Xd, o), (M, N), torch.float64)
    assert np.array_equal(Ct2, _run(gpu, lambda o: e1.exec_t(0, Xd, o), (M, N), torch.float64))
    for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        Xd, Yd = ops[dt]
        for mode in (0, 1):
            got = _run(gpu, lambda o: e2.sddmm(0, Xd, Yd, o, mode=mode), (nnz,), tdt)
            want = _run(gpu, lambda o: e1.sddmm(0, Xd, Yd, o, mode=mode), (nnz,), tdt)
            assert np.array_equal(got, want), (dt.__name__, mode)
    assert not e2.sddmm_built                                      # one grid column: no grid-row buffers, ever


def test_one_rank_update_values_doubles_every_product(crp, gpu, one_rank):
    """Twice the values: every product, partial sum and rounding doubles exactly (a power of two, no overflow), so exec, exec_t and
    the mode-1 SDDMM come out as exactly twice what they were."""
    import torch
    e2, _e1, va, ops = one_rank
    nnz = va.size
    Xd, Yd = ops[np.float64]
    calls = [(lambda o: e2.exec(0, Yd, o), (M, N), torch.float64), (lambda o: e2.exec_t(0, Xd, o), (M, N), torch.float64),
             (lambda o: e2.sddmm(0, Xd, Yd, o, mode=1), (nnz,), torch.float64),
             (lambda o: e2.sddmm(0, ops[np.float32][0], ops[np.float32][1], o, mode=1), (nnz,), torch.float32)]
    before = [_run(gpu, *c) for c in calls]
    e2.update_values(2.0 * va)
    after = [_run(gpu, *c) for c in calls]
    e2.update_values(va)
    for b, a in zip(before, after):
        assert np.abs(b).max() > 0 and np.array_equal(a, 2 * b)
    assert all(np.array_equal(_run(gpu, *c), b) for c, b in zip(calls, before))      # restored
    with pytest.raises(ValueError):
        e2.update_values(va[:-1])


def _worker(world, port, native):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    if native:
        env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        env["CRPSPMM_EXPECT_NATIVE_RCCL"] = "1"
        env.pop("CRPSPMM_EXCHANGE", None)
    else:
        env["CRPSPMM_EXCHANGE"] = "host"
        env.pop("CRPSPMM_EXPECT_NATIVE_RCCL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "gpu_dist_para2d_ops_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_PARA2D_OPS_WORKER_OK world=%d" % world in r.stdout


@pytest.mark.parametrize("world", [2, 4])
def test_every_grid_multi_rank_one_gpu(world):
    _worker(world, 29920 + world, native=False)


def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.parametrize("world", [2, 4])
def test_every_grid_native_rccl_multi_gpu(world):
    """The same worker with one rank per GPU and the native RCCL exchange; skipped on a box with fewer GPUs, as
    tests/test_gpu_dist.py::test_engines_native_rccl_multi_gpu is."""
    if _gpu_count() < world:
        pytest.skip("needs %d GPUs (native RCCL refuses two ranks on one device)" % world)
    _worker(world, 29930 + world, native=True)
