"""GPU: the sampled dense-dense product over A's pattern (csrc/sddmm_kernels.hip, crp_sddmm_csr_f64 / _f32) and the
row-parallel engine's SDDMM.

Error bound (derived, not measured).  With S = sum_j |x_j y_j| and unit roundoff u, any summation order of an n-term dot
product, with or without FMAs, errs by at most gamma_n S, gamma_n = n u / (1 - n u); one more rounding covers the scaling
of mode 1, and the fp32 path has one more again for the fp32 copy of the value.  Entry by entry, against np.longdouble
(own error <= n 2^-64 S):

    fp64 mode 0   (n + 1) u S         u = 2^-53          fp32 mode 0   (n + 1) u S         u = 2^-24
    fp64 mode 1   (n + 2) u |a| S                        fp32 mode 1   (n + 3) u |a| S

fp32 inputs follow the data rule of tests/fp32_ref.py (no result near the subnormal range); the reference is formed from
the fp32-rounded operands."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import FP64_TOL, ROOT
import fp32_ref

pytestmark = pytest.mark.gpu

U64, U32 = 2.0 ** -53, 2.0 ** -24


def _long_row_matrix(seed=2):
    """300 short rows (0 .. 5 entries) and, in their middle, one row that names every one of the 70 000 columns"""
    rng = np.random.default_rng(seed)
    ncol, nrow = 70000, 301
    lens = rng.integers(0, 6, nrow)
    lens[150] = ncol
    cols = [np.sort(rng.choice(ncol, size=l, replace=False)) if l < ncol else np.arange(ncol) for l in lens]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    return rp, ci, rng.standard_normal(ci.size), ncol


def _matrices():
    from crp_spmm_amd import gen
    rp, ci, va = gen.kkt3d(10)
    yield "kkt3d(10)", rp, ci, va, rp.size - 1
    rp, ci, va = gen.fem3d(7)
    yield "fem3d(7)", rp, ci, va, rp.size - 1
    rp, ci, va = gen.random_csr(3000, 1700, 40, empty_every=13)
    assert (np.diff(rp) == 0).any()
    yield "random_csr", rp, ci, va, 1700
    rp, ci, va, ncol = _long_row_matrix()
    yield "long_row", rp, ci, va, ncol


def _rows_of(rp):
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def _reference(rp, ci, X, Y, chunk=2048):
    """(ref, S) per nonzero in np.longdouble: ref = <X[i], Y[c]>, S = sum_j |x_j y_j|"""
    rows = _rows_of(rp)
    Xl, Yl = X.astype(np.longdouble), Y.astype(np.longdouble)
    ref = np.empty(ci.size, np.longdouble)
    S = np.empty(ci.size, np.longdouble)
    for a in range(0, ci.size, chunk):
        prod = Xl[rows[a:a + chunk]] * Yl[ci[a:a + chunk]]
        ref[a:a + chunk] = prod.sum(axis=1)
        S[a:a + chunk] = np.abs(prod).sum(axis=1)
    return ref, S


def _check(got, ref, bound, what):
    got = np.asarray(got).astype(np.longdouble)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got.astype(np.float64)).all(), (what, "non-finite output")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = int(np.argmax(ratio))
    print("%s: worst |got - ref| / bound = %.3g at nonzero %d" % (what, float(ratio[worst]), worst))
    assert (err <= bound).all(), (what, "bound missed at %d entries" % int((err > bound).sum()), float(ratio[worst]), worst)


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


@pytest.mark.parametrize("name_idx", range(4))
def test_parity_fp64(crp, gpu, name_idx):
    import torch
    from crp_spmm_amd import hip
    name, rp, ci, va, ncol = list(_matrices())[name_idx]
    nrow = rp.size - 1
    A = hip.CsrDev(nrow, ncol, rp, ci, va)
    for n in (1, 7, 24, 32, 33, 64, 100, 128, 256, 257, 512, 1000):
        rng = np.random.default_rng(1000 + n)
        X, Y = rng.standard_normal((nrow, n)), rng.standard_normal((ncol, n))
        Xd, Yd = _dev(gpu, X, Y)
        ref, S = _reference(rp, ci, X, Y)
        for mode in (0, 1):
            out = torch.full((ci.size,), float("nan"), dtype=torch.float64, device=gpu)
            A.sddmm(Xd, Yd, out=out, mode=mode)
            torch.cuda.synchronize()
            if mode == 0:
                _check(out.cpu().numpy(), ref, (n + 1) * U64 * S, (name, n, "fp64 mode 0"))
            else:
                a = va.astype(np.longdouble)
                _check(out.cpu().numpy(), a * ref, (n + 2) * U64 * np.abs(a) * S, (name, n, "fp64 mode 1"))
    A.free()


@pytest.mark.parametrize("name_idx", range(4))
def test_parity_fp32(crp, gpu, name_idx):
    import torch
    from crp_spmm_amd import hip
    name, rp, ci, _va, ncol = list(_matrices())[name_idx]
    nrow = rp.size - 1
    va = fp32_ref.data_values(np.random.default_rng(5), ci.size)
    A = hip.CsrDev(nrow, ncol, rp, ci, va)
    for n in (4, 30, 52, 128, 256, 1000):
        rng = np.random.default_rng(2000 + n)
        X, Y = fp32_ref.data_B(rng, (nrow, n)), fp32_ref.data_B(rng, (ncol, n))
        Xd, Yd = _dev(gpu, X, Y)
        ref, S = _reference(rp, ci, X, Y)
        for mode in (0, 1):
            out = torch.full((ci.size,), float("nan"), dtype=torch.float32, device=gpu)
            A.sddmm(Xd, Yd, out=out, mode=mode)
            torch.cuda.synchronize()
            if mode == 0:
                _check(out.cpu().numpy(), ref, (n + 1) * U32 * S, (name, n, "fp32 mode 0"))
            else:
                a = va.astype(np.longdouble)
                _check(out.cpu().numpy(), a * ref, (n + 3) * U32 * np.abs(a) * S, (name, n, "fp32 mode 1"))
    A.free()


def _strided(gpu, a, ld, offset):
    """a copy of the 2-D array a on the device with leading dimension ld, starting `offset` elements into its allocation"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    flat = torch.full((a.shape[0] * ld + offset + 8,), float("nan"), dtype=t.dtype, device=gpu)
    view = torch.as_strided(flat, a.shape, (ld, 1), storage_offset=offset)
    view.copy_(t)
    return view


FIXED_WIDTHS = {"f64": (1, 4, 7, 24, 32, 64, 100, 128, 130, 256, 300, 512, 600, 1000, 1100),
                "f32": (4, 7, 30, 64, 128, 200, 256, 512, 1000, 1100, 2100)}


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_fixed_order(crp, gpu, dt):
    """Bit-identical: aligned operands against ld = n + 1 and pointers one element off; one source against two; the full
    handle against two row-subset handles; two consecutive calls."""
    import torch
    from crp_spmm_amd import gen, hip
    ndt, tdt = (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)
    rp, ci, va = gen.random_csr(3000, 1700, 40, empty_every=13)
    nrow, ncol, nnz = 3000, 1700, ci.size
    rows = _rows_of(rp)
    A = hip.CsrDev(nrow, ncol, rp, ci, va)
    # the same columns with codes < 0 for the rows of Y from k0 on
    k0 = 900
    codes = np.where(ci < k0, ci, ~(ci - k0)).astype(np.int32)
    A2 = hip.CsrDev(nrow, k0, rp, codes, va)
    # two row subsets that cover the matrix: rows 0, 3, 4, 7, 8, ... and the rest
    pick = (np.arange(nrow) % 4) % 3 == 0
    subs = []
    for sel in (pick, ~pick):
        r = np.flatnonzero(sel)
        keep = sel[rows]
        h = hip.CsrDev(r.size, ncol, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], va[keep])
        h.set_rowmap(r, nrow)
        subs.append((h, torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)))
    SENT = -77.0
    for n in FIXED_WIDTHS[dt]:
        rng = np.random.default_rng(3000 + n)
        X, Y = rng.standard_normal((nrow, n)).astype(ndt), rng.standard_normal((ncol, n)).astype(ndt)
        Xd, Yd = _dev(gpu, X, Y)
        for mode in (0, 1):
            base = A.sddmm(Xd, Yd, mode=mode)
            again = A.sddmm(Xd, Yd, mode=mode)
            torch.cuda.synchronize()
            base = base.cpu().numpy()
            assert np.isfinite(base).all() and np.array_equal(again.cpu().numpy(), base), (n, mode, "two consecutive calls")
            # ld = n + 1, pointers one element into their allocations
            got = A.sddmm(_strided(gpu, X, n + 1, 1), _strided(gpu, Y, n + 1, 1), mode=mode)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), base), (n, mode, "ld = n + 1, offset pointers")
            # X aligned, Y not (and the other way round)
            got = A.sddmm(Xd, _strided(gpu, Y, n + 3, 0), mode=mode)
            got2 = A.sddmm(_strided(gpu, X, n, 1), Yd, mode=mode)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), base) and np.array_equal(got2.cpu().numpy(), base), (n, mode, "mixed alignment")
            # two sources, the second with its own leading dimension
            got = A2.sddmm(Xd, Yd[:k0], Y1=_strided(gpu, Y[k0:], n + 4, 0), mode=mode)
            got2 = A2.sddmm(Xd, Yd[:k0], Y1=_strided(gpu, Y[k0:], n + 5, 3), mode=mode)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), base) and np.array_equal(got2.cpu().numpy(), base), (n, mode, "two sources")
            # row subsets through set_rowmap + out_pos
            out = torch.full((nnz,), SENT, dtype=tdt, device=gpu)
            subs[0][0].sddmm(Xd, Yd, out=out, out_pos=subs[0][1], mode=mode)
            torch.cuda.synchronize()
            half = out.cpu().numpy()
            named = np.zeros(nnz, bool)
            named[subs[0][1].cpu().numpy()] = True
            assert np.array_equal(half[named], base[named]) and (half[~named] == SENT).all(), (n, mode, "first row subset")
            subs[1][0].sddmm(Xd, Yd, out=out, out_pos=subs[1][1], mode=mode)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), base), (n, mode, "row subsets")
    for h in [A, A2] + [s[0] for s in subs]:
        h.free()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_only_what_is_named_is_touched(crp, gpu, dt):
    import torch
    from crp_spmm_amd import gen, hip
    ndt, tdt = (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)
    rp, ci, va = gen.random_csr(3000, 1700, 40, empty_every=13)
    # no row names columns 5, 600 .. 640 and the last one
    drop = np.isin(ci, np.concatenate([[5, 1699], np.arange(600, 641)]))
    lens = np.diff(rp) - np.bincount(_rows_of(rp)[drop], minlength=3000)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci, va = ci[~drop], va[~drop]
    nrow, ncol, nnz = 3000, 1700, ci.size
    empty = np.diff(rp) == 0
    unnamed = ~np.isin(np.arange(ncol), ci)
    assert empty.sum() > 100 and unnamed.sum() >= 43
    A = hip.CsrDev(nrow, ncol, rp, ci, va)
    SENT, G = -77.0, 8
    for n in (7, 32, 100, 256, 600, 1100):
        rng = np.random.default_rng(4000 + n)
        X, Y = rng.standard_normal((nrow, n)).astype(ndt), rng.standard_normal((ncol, n)).astype(ndt)
        Xd, Yd = _dev(gpu, X, Y)
        clean = A.sddmm(Xd, Yd)
        Xn, Yn = X.copy(), Y.copy()
        Xn[empty] = np.nan
        Yn[unnamed] = np.nan
        Xd, Yd = _dev(gpu, Xn, Yn)
        for mode in (0, 1):
            buf = torch.full((nnz + 2 * G,), SENT, dtype=tdt, device=gpu)
            A.sddmm(Xd, Yd, out=buf[G:G + nnz], mode=mode)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert (got[:G] == SENT).all() and (got[G + nnz:] == SENT).all(), (n, mode, "guard elements")
            assert np.isfinite(got).all(), (n, mode)
            if mode == 0:
                assert np.array_equal(got[G:G + nnz], clean.cpu().numpy()), (n, "unchanged by NaN in unnamed rows")
    A.free()


def test_argument_errors_write_nothing(crp, gpu):
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    rp, ci, va = gen.random_csr(500, 300, 30, seed=3)
    nnz, n = ci.size, 16
    A = hip.CsrDev(500, 300, rp, ci, va)
    codes = np.where(ci < 200, ci, ~(ci - 200)).astype(np.int32)
    A2 = hip.CsrDev(500, 200, rp, codes, va)
    SENT = -77.0
    for fn, tdt in ((lib.crp_sddmm_csr_f64, torch.float64), (lib.crp_sddmm_csr_f32, torch.float32)):
        X = torch.ones((500, n), dtype=tdt, device=gpu)
        Y = torch.ones((300, n), dtype=tdt, device=gpu)
        out = torch.full((nnz,), SENT, dtype=tdt, device=gpu)
        pos = torch.arange(nnz, dtype=torch.int32, device=gpu)
        good = dict(A=A.handle, n=n, X=X.data_ptr(), ldX=n, Y0=Y.data_ptr(), ldY0=n, Y1=None, ldY1=0, out=out.data_ptr(),
                    out_pos=None, mode=0)

        def call(**kw):
            a = dict(good, **kw)
            rc = fn(a["A"], a["n"], a["X"], a["ldX"], a["Y0"], a["ldY0"], a["Y1"], a["ldY1"], a["out"], a["out_pos"], a["mode"], None)
            torch.cuda.synchronize()
            return rc
        bad = [dict(A=None), dict(X=None), dict(out=None), dict(Y0=None), dict(n=0), dict(n=-3), dict(ldX=n - 1), dict(ldY0=n - 1),
               dict(Y1=Y.data_ptr(), ldY1=n - 1), dict(mode=2), dict(mode=-1), dict(mode=2, out_pos=pos.data_ptr()),
               dict(A=A2.handle, Y1=None)]            # negative codes and no second source
        for kw in bad:
            rc = call(**kw)
            assert rc < 0, (fn.__name__, kw, rc)
            assert bool((out == SENT).all()), (fn.__name__, kw, "out was written")
        assert call() == 0 and bool((out == n).all())           # the good call, afterwards: every dot of ones is n
    A.free()
    A2.free()


def test_round_trip_into_update_values(crp, orc, gpu):
    """out of mode 0, still in HBM, becomes the matrix's values; the product then equals the oracle's with those values"""
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    for rp, ci, va, ncol in ((*gen.kkt3d(10), None), (*gen.random_csr(3000, 1700, 40, empty_every=13), 1700)):
        nrow = rp.size - 1
        ncol = nrow if ncol is None else ncol
        A = hip.CsrDev(nrow, ncol, rp, ci, va)
        n = 32
        rng = np.random.default_rng(7)
        X, Y = rng.standard_normal((nrow, n)), rng.standard_normal((ncol, n))
        Xd, Yd = _dev(gpu, X, Y)
        st = torch.cuda.current_stream().cuda_stream
        for nb in (24, 256):
            B = orc.fill_B(0, ncol, 0, nb)
            Bd = torch.from_numpy(B).to(gpu)
            Cd = torch.full((nrow, nb), float("nan"), dtype=torch.float64, device=gpu)
            hip.spmm_csr(A, Bd, Cd)                                         # the formats of this width exist before the update
            scores = A.sddmm(Xd, Yd)
            rc = lib.crp_csr_dev_update_values(A.handle, C.c_void_p(scores.data_ptr()), C.c_void_p(st))
            assert rc == 0
            hip.spmm_csr(A, Bd, Cd)
            torch.cuda.synchronize()
            err = orc.rel_fro_err(orc.spmm_csr(rp, ci, scores.cpu().numpy(), B), Cd.cpu().numpy())
            assert err <= FP64_TOL, (nrow, nb, err)
            A.update_values(va)
        A.free()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_engine_one_rank_matches_the_device_level_call(crp, gpu, dt):
    import torch
    from crp_spmm_amd import comm, engine, gen, hip
    ndt, tdt = (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)
    sc = comm.SelfComm()
    for rp, ci, va, k in ((*gen.random_csr(3000, 1700, 40, empty_every=13), 1700), (*gen.kkt3d(9), None)):
        m = rp.size - 1
        k = m if k is None else k
        A = hip.CsrDev(m, k, rp, ci, va)
        for n in (24, 257):
            e = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
            rng = np.random.default_rng(9)
            X, Y = rng.standard_normal((m, n)).astype(ndt), rng.standard_normal((k, n)).astype(ndt)
            Xd, Yd = _dev(gpu, X, Y)
            assert not e.sddmm_built
            for mode in (0, 1):
                want = A.sddmm(Xd, Yd, mode=mode)
                torch.cuda.synchronize()
                want = want.cpu().numpy()
                for timing in (True, False):
                    e.set_timing(timing)
                    out = torch.full((ci.size,), float("nan"), dtype=tdt, device=gpu)
                    e.sddmm(0, Xd, Yd, out, mode=mode)
                    torch.cuda.synchronize()
                    assert e.sddmm_built
                    assert np.array_equal(out.cpu().numpy(), want), (m, n, mode, timing, "device operands")
                    # column-major device operands
                    out.fill_(float("nan"))
                    e.sddmm(1, Xd.t().contiguous(), Yd.t().contiguous(), out, mode=mode)
                    torch.cuda.synchronize()
                    assert np.array_equal(out.cpu().numpy(), want), (m, n, mode, timing, "device operands, column-major")
                    # host operands, both layouts, host out
                    oh = np.full(ci.size, np.nan, ndt)
                    e.sddmm(0, X, Y, oh, mode=mode)
                    assert np.array_equal(oh, want), (m, n, mode, timing, "host operands")
                    oh = np.full(ci.size, np.nan, ndt)
                    e.sddmm(1, np.ascontiguousarray(X.T), np.ascontiguousarray(Y.T), oh, mode=mode)
                    assert np.array_equal(oh, want), (m, n, mode, timing, "host operands, column-major")
            e.free()
        A.free()
    sc.free()


@pytest.mark.parametrize("world", [2, 4])
def test_sddmm_multi_rank_one_gpu(world):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29880 + world), os.path.join(ROOT, "tests", "gpu_dist_sddmm_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_SDDMM_WORKER_OK world=%d" % world in r.stdout


def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.parametrize("world", [2, 4])
def test_sddmm_native_rccl_multi_gpu(world):
    """The same worker with one rank per GPU and the native RCCL exchange; skipped on a box with fewer GPUs, as
    tests/test_gpu_transpose.py::test_exec_t_native_rccl_multi_gpu is."""
    if _gpu_count() < world:
        pytest.skip("needs %d GPUs (native RCCL refuses two ranks on one device)" % world)
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env["CRPSPMM_EXPECT_NATIVE_RCCL"] = "1"
    env.pop("CRPSPMM_EXCHANGE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29890 + world), os.path.join(ROOT, "tests", "gpu_dist_sddmm_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_SDDMM_WORKER_OK world=%d" % world in r.stdout
