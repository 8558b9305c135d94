"""GPU: the row softmax over A's pattern and its Jacobian product (csrc/softmax_kernels.hip; crp_row_softmax_*,
crp_csr_dev_row_softmax_*, the engines' row_softmax).

Parity against np.longdouble inside the derived bounds of tests/softmax_ref.py (forward 1.01 (L + 2 T + 8) u ref, backward
1.01 u |y| ((L + 2) S + 2 |dy|)), on that module's inputs -- the ones tests/test_softmax_ref.py replays on the CPU; the special
cases exactly; the fixed summation order with np.array_equal throughout; that nothing but the named entries is touched; the
argument errors; the engines on one rank with the loop sddmm -> row_softmax -> update_values_dev -> exec closed in HBM; and 2
and 4 ranks sharing the GPU, every rank's result being its slice of the one-GPU result bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import softmax_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ("f64", "f32")


def _dt(dt):
    import torch
    return (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.array(a, order="C")).to(gpu) for a in arrays]


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _nan_like(gpu, n, tdt):
    import torch
    return torch.full((n,), float("nan"), dtype=tdt, device=gpu)


@pytest.mark.parametrize("name", R.PATTERNS + R.EDGE_PATTERNS)
@pytest.mark.parametrize("dt", DTYPES)
def test_parity_and_row_sums(crp, gpu, dt, name):
    from crp_spmm_amd import hip
    ndt, tdt = _dt(dt)
    u = R.U[np.dtype(ndt)]
    for pname, spread in R.parity_cases():
        if pname != name:
            continue
        rp, s, ref, bound, y, dy, ref_b, bound_b = R.case(name, spread, ndt)
        lens = np.diff(rp)
        rows = R.rows_of(rp)
        starts, ne = R._seg(rp)
        rp_d, s_d, y_d, dy_d = _dev(gpu, rp, s, y, dy)
        got = _host(hip.row_softmax(rp_d, s_d, out=_nan_like(gpu, s.size, tdt)))
        w, at = R.worst(got, ref, bound)
        print("%s %s spread %s: forward worst |err| / bound = %.3g at %d" % (name, dt, spread, w, at))
        assert np.isfinite(got).all(), (name, spread, "non-finite output")
        assert w <= 1.0, (name, spread, "forward bound missed", w, at)
        # the special cases, exactly
        assert (got[np.isneginf(s)] == 0).all(), (name, spread, "a masked entry is not exactly 0")
        assert (got[rp[:-1][lens == 1]] == 1).all(), (name, spread, "a row of one entry is not exactly 1")
        # every row sums to 1 within (L + 2 T + 8) u
        _ref, L, T = R.reference_fwd(rp, s)
        sums = np.add.reduceat(got.astype(np.longdouble), starts)
        tol = ((L + 2 * T + 8) * u)[starts]
        assert (np.abs(sums - 1) <= tol).all(), (name, spread, "row sums", float(np.max(np.abs(sums - 1) / tol)))
        # backward, from the y and dy of the case
        gb = _host(hip.row_softmax_bwd(rp_d, y_d, dy_d, out=_nan_like(gpu, s.size, tdt)))
        w, at = R.worst(gb, ref_b, bound_b)
        print("%s %s spread %s: backward worst |err| / bound = %.3g at %d" % (name, dt, spread, w, at))
        assert np.isfinite(gb).all(), (name, spread, "non-finite output")
        assert w <= 1.0, (name, spread, "backward bound missed", w, at)
        dsum = np.abs(np.add.reduceat(gb.astype(np.longdouble), starts))
        btot = np.add.reduceat(bound_b, starts)
        assert (dsum <= btot).all(), (name, spread, "row sums of ds", int(np.argmax(dsum - btot)))
        assert rows.size == s.size


@pytest.mark.parametrize("dt", DTYPES)
def test_masked_rows_and_nan_rows(crp, gpu, dt):
    """An all-masked row gives zeros and no NaN anywhere, on the register path and on the path over memory; a row that holds
    NaN or +inf leaves every other row's bits as they are without it, and nothing faults."""
    from crp_spmm_amd import hip
    ndt, tdt = _dt(dt)
    rp, s, _ref, _b, _y, dy, _rb, _bb = R.case("synthetic", 8, ndt)
    lens = np.diff(rp)
    rp_d, s_d, dy_d = _dev(gpu, rp, s, dy)
    clean = _host(hip.row_softmax(rp_d, s_d))
    clean_d = _dev(gpu, clean)[0]
    clean_b = _host(hip.row_softmax_bwd(rp_d, clean_d, dy_d))
    assert np.isfinite(clean).all() and np.isfinite(clean_b).all()
    pick = [int(np.flatnonzero(lens == L)[0]) for L in (1, 3, 64, 100, 200, 513, 4097)]
    s2 = s.copy()
    for r in pick:
        s2[rp[r]:rp[r + 1]] = -np.inf
    got = _host(hip.row_softmax(rp_d, _dev(gpu, s2)[0], out=_nan_like(gpu, s.size, tdt)))
    assert not np.isnan(got).any()
    touched = np.isin(R.rows_of(rp), pick)
    assert (got[touched] == 0).all() and np.array_equal(got[~touched], clean[~touched])
    for poison in (np.nan, np.inf):
        s3 = s.copy()
        for r in pick:
            s3[rp[r] + (rp[r + 1] - rp[r]) // 2] = poison
        got = _host(hip.row_softmax(rp_d, _dev(gpu, s3)[0], out=_nan_like(gpu, s.size, tdt)))
        assert np.array_equal(got[~touched], clean[~touched]), poison
        dy3 = dy.copy()
        for r in pick:
            dy3[rp[r] + (rp[r + 1] - rp[r]) // 2] = poison
        gb = _host(hip.row_softmax_bwd(rp_d, clean_d, _dev(gpu, dy3)[0], out=_nan_like(gpu, s.size, tdt)))
        assert np.array_equal(gb[~touched], clean_b[~touched]), (poison, "backward")


def _np_transpose_rowptr(ci, ncol):
    return np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncol))]).astype(np.int32)


@pytest.mark.parametrize("dt", DTYPES)
def test_fixed_order(crp, gpu, dt):
    import torch
    from crp_spmm_amd import hip
    ndt, tdt = _dt(dt)
    for name in ("synthetic", "random_csr"):
        rp, s, _ref, _b, y, dy, _rb, _bb = R.case(name, "max", ndt)
        nnz, nrow = s.size, rp.size - 1
        rp_d, s_d, y_d, dy_d = _dev(gpu, rp, s, y, dy)
        base = _host(hip.row_softmax(rp_d, s_d))
        base_b = _host(hip.row_softmax_bwd(rp_d, y_d, dy_d))
        assert np.isfinite(base).all() and np.isfinite(base_b).all()
        # repeated calls
        assert np.array_equal(_host(hip.row_softmax(rp_d, s_d)), base), (name, "two calls")
        assert np.array_equal(_host(hip.row_softmax_bwd(rp_d, y_d, dy_d)), base_b), (name, "two calls, backward")
        # every array one element into its allocation: the result does not depend on alignment
        off = lambda a: torch.cat([a[:1], a])[1:]
        assert off(s_d).data_ptr() % 16 != s_d.data_ptr() % 16
        got = torch.full((nnz + 1,), float("nan"), dtype=tdt, device=gpu)
        hip.row_softmax(rp_d, s_d, out=got[1:])
        assert np.array_equal(_host(got)[1:], base), (name, "out one element off")
        hip.row_softmax(rp_d, off(s_d), out=got[1:])
        assert np.array_equal(_host(got)[1:], base), (name, "s and out one element off")
        hip.row_softmax_bwd(rp_d, off(y_d), dy_d, out=got[1:])
        assert np.array_equal(_host(got)[1:], base_b), (name, "backward, y and out one element off")
        hip.row_softmax_bwd(rp_d, y_d, off(dy_d), out=got[1:])
        assert np.array_equal(_host(got)[1:], base_b), (name, "backward, dy and out one element off")
        assert np.isnan(_host(got)[0])
        # in place
        t = s_d.clone()
        assert hip.row_softmax(rp_d, t, out=t) is t and np.array_equal(_host(t), base), (name, "y == s")
        t = dy_d.clone()
        hip.row_softmax_bwd(rp_d, y_d, t, out=t)
        assert np.array_equal(_host(t), base_b), (name, "ds == dy")
        t = y_d.clone()
        hip.row_softmax_bwd(rp_d, t, dy_d, out=t)
        assert np.array_equal(_host(t), base_b), (name, "ds == y")
        # rowptr + r0: row subsets of the same arrays, and nothing outside them
        for r0, r1 in ((0, nrow // 3), (nrow // 3, nrow - 5), (nrow - 5, nrow), (7, 8), (nrow // 2, nrow // 2)):
            lo, hi = int(rp[r0]), int(rp[r1])
            got = _host(hip.row_softmax(rp_d[r0:r1 + 1], s_d, out=_nan_like(gpu, nnz, tdt)))
            assert np.array_equal(got[lo:hi], base[lo:hi]), (name, r0, r1)
            assert np.isnan(got[:lo]).all() and np.isnan(got[hi:]).all(), (name, r0, r1, "outside the subset")
            got = _host(hip.row_softmax_bwd(rp_d[r0:r1 + 1], y_d, dy_d, out=_nan_like(gpu, nnz, tdt)))
            assert np.array_equal(got[lo:hi], base_b[lo:hi]), (name, r0, r1, "backward")
            assert np.isnan(got[:lo]).all() and np.isnan(got[hi:]).all(), (name, r0, r1, "backward, outside the subset")


@pytest.mark.parametrize("dt", DTYPES)
def test_the_same_rows_under_every_lane_group(crp, gpu, dt):
    """The rows of the synthetic row pointer inside row pointers whose mean row length selects the 8-, 16-, 32- and 64-lane
    instance (short neighbours only ... the 70 000-entry row and rows of about 200 entries): the same bits everywhere."""
    from crp_spmm_amd import hip
    ndt, tdt = _dt(dt)
    rp0, s0, _ref, _b, y0, dy0, _rb, _bb = R.case("synthetic", "max", ndt)
    n0 = s0.size
    rp_d, s_d, y_d, dy_d = _dev(gpu, rp0, s0, y0, dy0)
    base, base_b = _host(hip.row_softmax(rp_d, s_d)), _host(hip.row_softmax_bwd(rp_d, y_d, dy_d))
    big = np.concatenate([R.SYNTH_LENGTHS, [70000], np.arange(190, 211)])
    neighbours = [(name, R.pattern(name)) for name in R.EDGE_PATTERNS] + [("long neighbours", R.rowptr_of(big))]
    seen = {R.lpr_of(rp0)}
    for name, rp in neighbours:
        assert np.array_equal(rp[:rp0.size], rp0)
        seen.add(R.lpr_of(rp))
        extra = int(rp[-1]) - n0
        tail = R.scores(R.rowptr_of(np.diff(rp)[rp0.size - 1:]), ndt, 8, 5)
        assert tail.size == extra
        s = np.concatenate([s0, tail])
        y = np.concatenate([y0, np.full(extra, 1.0 / 8, ndt)])
        dy = np.concatenate([dy0, R.grads(extra, ndt, 6)])
        rd, sd, yd, dyd = _dev(gpu, rp, s, y, dy)
        got = _host(hip.row_softmax(rd, sd, out=_nan_like(gpu, s.size, tdt)))
        assert np.array_equal(got[:n0], base), (name, R.lpr_of(rp))
        assert np.isfinite(got).all()
        got = _host(hip.row_softmax_bwd(rd, yd, dyd, out=_nan_like(gpu, s.size, tdt)))
        assert np.array_equal(got[:n0], base_b), (name, R.lpr_of(rp), "backward")
    assert seen == {8, 16, 32, 64}


@pytest.mark.parametrize("dt", DTYPES)
def test_handle_forms_equal_the_raw_forms(crp, gpu, dt):
    from crp_spmm_amd import gen, hip
    ndt, tdt = _dt(dt)
    rp, ci, va = gen.random_csr(3000, 1700, 40, empty_every=13)
    nnz = ci.size
    rp_t = _np_transpose_rowptr(ci, 1700)
    A, At = hip.CsrDev(3000, 1700, rp, ci, va), hip.CsrDev.from_transpose(3000, 1700, rp, ci, va)
    assert At.is_transposed and At.nnz == nnz
    for h, p in ((A, rp), (At, rp_t)):
        s = R.scores(p, ndt, 8, 11)
        y = R.replay_fwd(p, s)
        dy = R.grads(nnz, ndt, 12)
        p_d, s_d, y_d, dy_d = _dev(gpu, p, s, y, dy)
        assert np.array_equal(_host(h.row_softmax(s_d)), _host(hip.row_softmax(p_d, s_d)))
        assert np.array_equal(_host(h.row_softmax_bwd(y_d, dy_d)), _host(hip.row_softmax_bwd(p_d, y_d, dy_d)))
        t = s_d.clone()
        assert h.row_softmax(t, out=t) is t and np.array_equal(_host(t), _host(hip.row_softmax(p_d, s_d)))
        with pytest.raises(ValueError):
            h.row_softmax(s_d[:-1])
        with pytest.raises(TypeError):
            h.row_softmax_bwd(y_d, dy_d.double() if dt == "f32" else dy_d.float())
    A.free()
    At.free()


@pytest.mark.parametrize("dt", DTYPES)
def test_only_what_is_named_is_touched(crp, gpu, dt):
    """rowptr[0] = G > 0: G guard entries of NaN before the first row's entries and after the last row's, in every array; a
    matrix with empty rows; the outputs pre-filled with NaN."""
    from crp_spmm_amd import hip
    ndt, tdt = _dt(dt)
    rp, s, _ref, _b, y, dy, _rb, _bb = R.case("random_csr", 8, ndt)
    assert (np.diff(rp) == 0).sum() > 100
    nnz, G = s.size, 9
    rp_d, s_d, y_d, dy_d = _dev(gpu, rp, s, y, dy)
    base, base_b = _host(hip.row_softmax(rp_d, s_d)), _host(hip.row_softmax_bwd(rp_d, y_d, dy_d))
    guard = lambda a: np.concatenate([np.full(G, np.nan, ndt), a, np.full(G, np.nan, ndt)])
    rg_d, sg_d, yg_d, dyg_d = _dev(gpu, (rp + G).astype(np.int32), guard(s), guard(y), guard(dy))
    got = _host(hip.row_softmax(rg_d, sg_d, out=_nan_like(gpu, nnz + 2 * G, tdt)))
    assert np.isnan(got[:G]).all() and np.isnan(got[G + nnz:]).all() and np.array_equal(got[G:G + nnz], base)
    got = _host(hip.row_softmax_bwd(rg_d, yg_d, dyg_d, out=_nan_like(gpu, nnz + 2 * G, tdt)))
    assert np.isnan(got[:G]).all() and np.isnan(got[G + nnz:]).all() and np.array_equal(got[G:G + nnz], base_b)
    # in place, the guards of the input survive
    hip.row_softmax(rg_d, sg_d, out=sg_d)
    got = _host(sg_d)
    assert np.isnan(got[:G]).all() and np.isnan(got[G + nnz:]).all() and np.array_equal(got[G:G + nnz], base)


def test_argument_errors_write_nothing(crp, gpu):
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    rp, ci, va = gen.fem3d(7)
    rp = rp.astype(np.int32)
    nrow, nnz = rp.size - 1, int(rp[-1])
    rp_d = _dev(gpu, rp)[0]
    A = hip.CsrDev(nrow, nrow, rp, ci, va)
    SENT = -77.0
    for sfx, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        a = torch.zeros(nnz, dtype=tdt, device=gpu)
        out = torch.full((nnz,), SENT, dtype=tdt, device=gpu)
        fwd, bwd = getattr(lib, "crp_row_softmax_" + sfx), getattr(lib, "crp_row_softmax_bwd_" + sfx)
        hf, hb = getattr(lib, "crp_csr_dev_row_softmax_" + sfx), getattr(lib, "crp_csr_dev_row_softmax_bwd_" + sfx)
        p, q, o = rp_d.data_ptr(), a.data_ptr(), out.data_ptr()
        calls = [(lambda: fwd(-1, p, q, o, None), -1), (lambda: fwd(nrow, None, q, o, None), -1), (lambda: fwd(nrow, p, None, o, None), -1),
                 (lambda: fwd(0, p, q, o, None), 0), (lambda: fwd(0, None, None, None, None), 0),
                 (lambda: bwd(-5, p, q, q, o, None), -1), (lambda: bwd(nrow, None, q, q, o, None), -1),
                 (lambda: bwd(nrow, p, None, q, o, None), -1), (lambda: bwd(nrow, p, q, None, o, None), -1),
                 (lambda: bwd(0, p, q, q, o, None), 0),
                 (lambda: hf(None, q, o, None), -1), (lambda: hf(A.handle, None, o, None), -1),
                 (lambda: hb(None, q, q, o, None), -1), (lambda: hb(A.handle, None, q, o, None), -1), (lambda: hb(A.handle, q, None, o, None), -1)]
        for i, (call, want) in enumerate(calls):
            rc = call()
            torch.cuda.synchronize()
            assert rc == want, (sfx, i, rc)
            assert bool((out == SENT).all()), (sfx, i, "out was written")
        assert fwd(nrow, p, q, None, None) == -1 and hf(A.handle, q, None, None) == -1 and bwd(nrow, p, q, q, None, None) == -1
        assert hf(A.handle, q, o, None) == 0                      # the good call, afterwards: equal scores give 1 / L
        lens = np.diff(rp)
        want = (np.ones(nnz, a.cpu().numpy().dtype) / np.repeat(lens, lens).astype(a.cpu().numpy().dtype))
        assert np.array_equal(_host(out), want)
    A.free()


@pytest.mark.parametrize("dt", DTYPES)
def test_engine_one_rank_and_the_closed_loop(crp, gpu, dt):
    """RpSpmm / Para2dSpmm (1 x 1) row_softmax equal the device-level call bit for bit; the upload happens in the first call;
    sddmm(mode 0) -> row_softmax -> update_values_dev -> exec on the device equals, bit for bit, exec after a host
    update_values with the downloaded y (fp32: widened)."""
    import torch
    from crp_spmm_amd import comm, engine, gen, hip
    ndt, tdt = _dt(dt)
    sc = comm.SelfComm()
    for rp, ci, va, k in ((*gen.random_csr(3000, 1700, 40, empty_every=13), 1700), (*gen.kkt3d(9), None)):
        m, nnz, n = rp.size - 1, ci.size, 24
        k = m if k is None else k
        rp_d = _dev(gpu, rp.astype(np.int32))[0]
        ea = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
        eb = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
        e2 = engine.Para2dSpmm(sc, 1, 1, [0, m], [0, k], [0, m], [0, n], rp, ci, va)
        rng = np.random.default_rng(21)
        X, Y, B = (rng.uniform(-1, 1, sh).astype(ndt) for sh in ((m, n), (k, n), (k, n)))
        Xd, Yd, Bd = _dev(gpu, X, Y, B)
        s = _nan_like(gpu, nnz, tdt)
        ea.sddmm(0, Xd, Yd, s)
        assert not ea.row_softmax_built and not e2.row_softmax_built
        y = ea.row_softmax(s)
        assert ea.row_softmax_built and not eb.row_softmax_built
        want = _host(hip.row_softmax(rp_d, s))
        assert np.array_equal(_host(y), want) and np.isfinite(want).all()
        assert np.array_equal(_host(e2.row_softmax(s)), want) and e2.row_softmax_built and e2.rp.row_softmax_built
        dy = _dev(gpu, R.grads(nnz, ndt, 22))[0]
        want_b = _host(hip.row_softmax_bwd(rp_d, y, dy))
        assert np.array_equal(_host(ea.row_softmax_bwd(y, dy)), want_b)
        assert np.array_equal(_host(e2.row_softmax_bwd(y, dy, out=_nan_like(gpu, nnz, tdt))), want_b)
        t = dy.clone()
        assert ea.row_softmax_bwd(y, t, out=t) is t and np.array_equal(_host(t), want_b)
        with pytest.raises(ValueError):
            ea.row_softmax(s[:-1])
        # the loop closed in HBM against the loop through the host
        Ca, Cb = (torch.full((m, n), float("nan"), dtype=tdt, device=gpu) for _ in range(2))
        ea.set_timing(False)
        ea.sddmm(0, Xd, Yd, s)
        ea.row_softmax(s, out=s)
        ea.update_values_dev(s)
        ea.exec(0, Bd, Ca)
        eb.update_values(want.astype(np.float64))
        eb.exec(0, Bd, Cb)
        ca = _host(Ca)
        assert np.array_equal(_host(s), want)
        assert not np.isnan(ca).any() and np.abs(ca).max() > 0 and np.array_equal(ca, _host(Cb))
        for e in (ea, eb, e2):
            e.free()
    sc.free()


def _worker(script, ok, world, port, native):
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
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", script)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%s world=%d" % (ok, world) in r.stdout


WORKERS = {"rp": ("gpu_dist_softmax_worker.py", "GPU_DIST_SOFTMAX_WORKER_OK", 30040),
           "para2d": ("gpu_dist_para2d_softmax_worker.py", "GPU_DIST_PARA2D_SOFTMAX_WORKER_OK", 30060)}


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("which", sorted(WORKERS))
def test_multi_rank_one_gpu(which, world):
    script, ok, port = WORKERS[which]
    _worker(script, ok, world, port + world, native=False)


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
    tests/test_gpu_sddmm.py::test_sddmm_native_rccl_multi_gpu is."""
    if _gpu_count() < world:
        pytest.skip("needs %d GPUs (native RCCL refuses two ranks on one device)" % world)
    script, ok, port = WORKERS[which]
    _worker(script, ok, world, port + 10 + world, native=True)
