"""GPU: the fused backward of the sparse attention (csrc/attention_bwd_kernels.hip, crp_attention_bwd_q_csr_* /
crp_attention_bwd_kv_csr_*), its Python wrappers and hip.sparse_attention.  Reference, bounds (derived in DESIGN.md 5l) and
data: tests/attention_bwd_ref.py."""
import numpy as np
import pytest

import attention_bwd_ref as B
import attention_ref as R
from test_gpu_attention import SENT, _dev, _strided, _tdt

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
KEYS = ("dQ", "dK", "dV", "ds", "delta")


def _handles(rp, ci, nrow, ncol, val=None):
    from crp_spmm_amd import hip
    val = np.ones(ci.size) if val is None else val
    return hip.CsrDev(nrow, ncol, rp, ci, val), hip.CsrDev.from_transpose(nrow, ncol, rp, ci, val)


def _forward(A, gpu, Qd, Kd, Vd, scale, bias=False):
    import torch
    lse = torch.full((Qd.shape[0],), float("nan"), dtype=Qd.dtype, device=gpu)
    O = A.attention(Qd, Kd, Vd, scale=scale, bias=bias, lse=lse)
    return O, lse


def _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale, bias=False, want_ds=True):
    """both calls -> dict of numpy arrays (ds None when not asked for)"""
    import torch
    ds = torch.full((max(A.nnz, 1),), float("nan"), dtype=Qd.dtype, device=gpu)[:A.nnz] if want_ds else None
    dQ, delta = A.attention_bwd_q(Qd, Kd, Vd, Od, dOd, lsed, scale=scale, bias=bias, ds_out=ds)
    dK, dV = At.attention_bwd_kv(Kd, Vd, Qd, dOd, lsed, delta, scale=scale, bias=bias)
    torch.cuda.synchronize()
    return dict(dQ=dQ.cpu().numpy(), dK=dK.cpu().numpy(), dV=dV.cpu().numpy(), ds=None if ds is None else ds.cpu().numpy(),
                delta=delta.cpu().numpy())


def _same(a, b, what):
    for k in a:
        if a[k] is not None and b.get(k) is not None:
            assert np.array_equal(a[k], b[k]) and np.array_equal(np.signbit(a[k]), np.signbit(b[k])), (what, k)


@pytest.mark.parametrize("nk,nv,dtype", list(B.parity_cases()))
def test_parity(crp, gpu, nk, nv, dtype):
    """either side of every instance threshold and at the cap; rows of 0, 1, 7, 8, 9, 63, 64, 65 and 200 entries, columns of 0, 1,
    8 and 9 and the hub of > 2000 (the wide cases: the short rows)"""
    rp, ci, nrow, Q, K, V, dO, scale, ref = B.case(nk, nv, dtype)
    A, At = _handles(rp, ci, nrow, B.NCOL)
    Qd, Kd, Vd, dOd = _dev(gpu, Q, K, V, dO)
    Od, lsed = _forward(A, gpu, Qd, Kd, Vd, scale)
    got = _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale)
    w = B.ratios(got, ref, dtype)
    print("parity %s nk=%d nv=%d %s: worst |got - ref| / bound  %s" % (dtype, nk, nv, R.lpr_of(nk, nv, dtype),
                                                                      "  ".join("%s %.3g" % (k, w[k]) for k in KEYS)))
    assert all(w[k] <= 1 for k in KEYS), w
    empty = np.diff(rp) == 0
    assert (got["dQ"][empty] == 0).all() and not np.signbit(got["dQ"][empty]).any()
    nocol = np.bincount(ci, minlength=B.NCOL) == 0
    assert nocol.any()
    for k in ("dK", "dV"):
        assert (got[k][nocol] == 0).all() and not np.signbit(got[k][nocol]).any()
    one = np.flatnonzero(np.diff(rp) == 1)
    assert (got["ds"][rp[one]] == 0).all() and not np.signbit(got["ds"][rp[one]]).any(), "a one-entry row: p = 1, dP = delta"
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_over_the_cap_returns_its_code_and_writes_nothing(crp, gpu, dtype):
    import torch
    lib = crp.load()
    tdt = _tdt(dtype)
    cap = B.CAP[np.dtype(dtype)]
    rp, ci, nrow = B.matrix(short=True)
    A, At = _handles(rp, ci, nrow, B.NCOL)
    sfx = "f64" if dtype == "float64" else "f32"
    fq, fkv = getattr(lib, "crp_attention_bwd_q_csr_" + sfx), getattr(lib, "crp_attention_bwd_kv_csr_" + sfx)
    for nk, nv in ((cap + 1, 8), (8, cap + 1)):
        Q = torch.ones((nrow, nk), dtype=tdt, device=gpu)
        K = torch.ones((B.NCOL, nk), dtype=tdt, device=gpu)
        V = torch.ones((B.NCOL, nv), dtype=tdt, device=gpu)
        O = torch.ones((nrow, nv), dtype=tdt, device=gpu)
        lse = torch.zeros((nrow,), dtype=tdt, device=gpu)
        outs = [torch.full(s, SENT, dtype=tdt, device=gpu) for s in ((nrow, nk), (nrow,), (ci.size,), (B.NCOL, nk), (B.NCOL, nv))]
        dQ, delta, ds, dK, dV = outs
        rc = fq(A.handle, nk, nv, 1.0, 0, Q.data_ptr(), nk, K.data_ptr(), nk, None, 0, V.data_ptr(), nv, None, 0, O.data_ptr(), nv,
                O.data_ptr(), nv, lse.data_ptr(), dQ.data_ptr(), nk, delta.data_ptr(), ds.data_ptr(), None, None)
        assert rc == B.EWIDTH, (nk, nv, rc)
        rc = fkv(At.handle, nk, nv, 1.0, 0, K.data_ptr(), nk, V.data_ptr(), nv, Q.data_ptr(), nk, O.data_ptr(), nv, lse.data_ptr(),
                 lse.data_ptr(), dK.data_ptr(), nk, dV.data_ptr(), nv, None)
        assert rc == B.EWIDTH, (nk, nv, rc)
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in outs), "something was written"
        with pytest.raises(ValueError):
            A.attention_bwd_q(Q, K, V, O, O, lse)
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_cases(crp, gpu, dtype):
    """masked edges (bias -inf) give exact zeros; all-masked and empty rows give +0, not NaN; a one-entry row gives dS = +0 and
    dV[c] = dO[i] bit for bit; the rescale-style rows of attention_ref.steep_case stay inside the bounds"""
    import torch
    dt = np.dtype(dtype)
    # rows: 0 empty, 1 one entry (column 9, which no other row names), 2 all masked, 3 .. 11 every second entry masked
    lens = [0, 1, 5] + [3, 8, 9, 16, 17, 24, 40, 12, 7]
    rng = np.random.default_rng(4)
    ncol = 64
    pool = np.setdiff1d(np.arange(ncol), [9, 33])                   # 33: a column only masked entries name
    cols, bias = [np.zeros(0, np.int64), np.array([9])], [np.zeros(0), np.zeros(1)]
    for r, n in enumerate(lens[2:], 2):
        c = np.sort(rng.choice(pool, size=n, replace=False))
        b = np.full(n, -np.inf) if r == 2 else np.where(np.arange(n) % 2 == 1, -np.inf, 0.25 * np.arange(n))
        if r in (5, 8):                                             # ... and column 33 in place of their first masked entry
            c[1] = 33
            order = np.argsort(c)
            c, b = c[order], b[order]
        cols.append(c)
        bias.append(b)
    rp = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    bias = np.concatenate(bias)
    nrow = rp.size - 1
    nk, nv = 24, 20
    Q, K, V, dO, scale = B.operands(nk, nv, dt, 31, nrow=nrow, ncol=ncol)
    ref = B.reference(rp, ci, Q, K, V, dO, scale, bias.astype(dt))
    A, At = _handles(rp, ci, nrow, ncol, bias)
    Qd, Kd, Vd, dOd = _dev(gpu, Q, K, V, dO)
    Od, lsed = _forward(A, gpu, Qd, Kd, Vd, scale, bias=True)
    got = _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale, bias=True)
    w = B.ratios(got, ref, dtype)
    print("special %s: %s" % (dtype, w))
    assert all(w[k] <= 1 for k in KEYS), w
    masked = ~np.isfinite(bias)
    assert (got["ds"][masked] == 0).all() and not np.signbit(got["ds"][masked]).any()
    for r in (0, 2):                                                # the empty and the all-masked row
        assert (got["dQ"][r] == 0).all() and not np.signbit(got["dQ"][r]).any()
    assert (got["dK"][33] == 0).all() and (got["dV"][33] == 0).all(), "a column only masked entries name"
    assert got["ds"][rp[1]] == 0 and not np.signbit(got["ds"][rp[1]])
    assert np.array_equal(got["dV"][9], dO[1]), "dV of the one-entry row's column is its dO row"
    assert (got["dK"][9] == 0).all()
    A.free()
    At.free()
    # the rescale-style rows
    rp, ci, bias, Q, K, V, scale, _ = R.steep_case(dtype)
    dO = np.random.default_rng(9).standard_normal((Q.shape[0], V.shape[1])).astype(dt)
    ref = B.reference(rp, ci, Q, K, V, dO, scale, bias.astype(dt))
    A, At = _handles(rp, ci, Q.shape[0], K.shape[0], bias)
    Qd, Kd, Vd, dOd = _dev(gpu, Q, K, V, dO)
    Od, lsed = _forward(A, gpu, Qd, Kd, Vd, scale, bias=True)
    got = _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale, bias=True)
    w = B.ratios(got, ref, dtype)
    print("steep rows %s: %s" % (dtype, w))
    assert all(w[k] <= 1 for k in KEYS), w
    assert (got["ds"][~np.isfinite(bias)] == 0).all()
    A.free()
    At.free()


FIXED = {"float64": ((3, 5), (17, 17), (33, 32), (8, 40), (65, 65), (129, 128)),
         "float32": ((3, 5), (33, 33), (65, 64), (8, 40), (129, 129), (257, 256))}


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_order(crp, gpu, dtype):
    """bit-identical across offsets, odd leading dimensions and unaligned pointers; row-subset handles on both sides; two-source K /
    V in bwd_q; with or without ds_out; repeated calls; in-place dK == K, dV == V against out-of-place"""
    import torch
    from crp_spmm_amd import hip
    tdt = _tdt(dtype)
    rp, ci, nrow = B.matrix()
    rows = R.rows_of(rp)
    rpt, cit, tmap = B.transpose(rp, ci, B.NCOL)
    A, At = _handles(rp, ci, nrow, B.NCOL)
    for nk, nv in FIXED[dtype]:
        Q, K, V, dO, scale = B.operands(nk, nv, dtype, 3 * nk + nv)
        Qd, Kd, Vd, dOd = _dev(gpu, Q, K, V, dO)
        Od, lsed = _forward(A, gpu, Qd, Kd, Vd, scale)
        base = _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale)
        assert all(np.isfinite(base[k]).all() for k in KEYS)
        _same(base, _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale), (dtype, nk, nv, "repeated"))
        _same(base, _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale, want_ds=False), (dtype, nk, nv, "without ds_out"))
        # odd leading dimensions, offsets that break the 16-byte alignment (inputs and outputs)
        for ld_extra, off in ((1, 0), (4, 1), (3, 3)):
            sQ, sK, sV, sO, sdO = (_strided(gpu, x, x.shape[1] + ld_extra, off) for x in (Q, K, V, Od.cpu().numpy(), dO))
            dQ = _strided(gpu, np.zeros((nrow, nk), dtype), nk + ld_extra, off)
            dK = _strided(gpu, np.zeros((B.NCOL, nk), dtype), nk + ld_extra, off)
            dV = _strided(gpu, np.zeros((B.NCOL, nv), dtype), nv + ld_extra, off)
            ds = torch.empty((ci.size,), dtype=tdt, device=gpu)
            _, delta = A.attention_bwd_q(sQ, sK, sV, sO, sdO, lsed, scale=scale, dQ=dQ, ds_out=ds)
            At.attention_bwd_kv(sK, sV, sQ, sdO, lsed, delta, scale=scale, dK=dK, dV=dV)
            torch.cuda.synchronize()
            got = dict(dQ=dQ.cpu().numpy(), dK=dK.cpu().numpy(), dV=dV.cpu().numpy(), ds=ds.cpu().numpy(), delta=delta.cpu().numpy())
            _same(base, got, (dtype, nk, nv, "ld + %d, offset %d" % (ld_extra, off)))
        # in place over K and V
        Kc, Vc = Kd.clone(), Vd.clone()
        delta = torch.from_numpy(base["delta"]).to(gpu)
        At.attention_bwd_kv(Kc, Vc, Qd, dOd, lsed, delta, scale=scale, dK=Kc, dV=Vc)
        torch.cuda.synchronize()
        _same(dict(dK=base["dK"], dV=base["dV"]), dict(dK=Kc.cpu().numpy(), dV=Vc.cpu().numpy()), (dtype, nk, nv, "in place"))
        # two sources in bwd_q
        k0 = 300
        codes = np.where(ci < k0, ci, ~(ci - k0)).astype(np.int32)
        A2 = hip.CsrDev(nrow, k0, rp, codes, np.ones(ci.size))
        ds = torch.empty((ci.size,), dtype=tdt, device=gpu)
        dQ, delta = A2.attention_bwd_q(Qd, Kd[:k0], Vd[:k0], Od, dOd, lsed, K1=Kd[k0:], V1=Vd[k0:], scale=scale, ds_out=ds)
        torch.cuda.synchronize()
        _same(base, dict(dQ=dQ.cpu().numpy(), delta=delta.cpu().numpy(), ds=ds.cpu().numpy()), (dtype, nk, nv, "two sources"))
        A2.free()
        # row subsets on both sides
        dQ = torch.full((nrow, nk), float("nan"), dtype=tdt, device=gpu)
        delta = torch.full((nrow,), float("nan"), dtype=tdt, device=gpu)
        ds = torch.full((ci.size,), float("nan"), dtype=tdt, device=gpu)
        pick = (np.arange(nrow) % 4) % 3 == 0
        for sel in (pick, ~pick):
            r = np.flatnonzero(sel)
            keep = sel[rows]
            h = hip.CsrDev(r.size, B.NCOL, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], np.ones(int(keep.sum())))
            h.set_rowmap(r, nrow)
            pos = torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)
            h.attention_bwd_q(Qd, Kd, Vd, Od, dOd, lsed, scale=scale, dQ=dQ, delta=delta, ds_out=ds, out_pos=pos)
            torch.cuda.synchronize()
            h.free()
        _same(base, dict(dQ=dQ.cpu().numpy(), delta=delta.cpu().numpy(), ds=ds.cpu().numpy()), (dtype, nk, nv, "row subsets of A"))
        dK = torch.full((B.NCOL, nk), float("nan"), dtype=tdt, device=gpu)
        dV = torch.full((B.NCOL, nv), float("nan"), dtype=tdt, device=gpu)
        trows = R.rows_of(rpt)
        pickc = np.arange(B.NCOL) % 3 == 1
        pickc[B.HUB] = True
        for sel in (pickc, ~pickc):
            r = np.flatnonzero(sel)
            keep = sel[trows]
            h = hip.CsrDev(r.size, nrow, np.concatenate([[0], np.cumsum(np.diff(rpt)[r])]).astype(np.int32), cit[keep], np.ones(int(keep.sum())))
            h.set_rowmap(r, B.NCOL)
            h.attention_bwd_kv(Kd, Vd, Qd, dOd, lsed, delta, scale=scale, dK=dK, dV=dV)
            torch.cuda.synchronize()
            h.free()
        _same(dict(dK=base["dK"], dV=base["dV"]), dict(dK=dK.cpu().numpy(), dV=dV.cpu().numpy()), (dtype, nk, nv, "row subsets of A^T"))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_only_what_is_named_is_touched(crp, gpu, dtype):
    """guard bands around every output and the pad columns of dQ, dK, dV keep their sentinel; K / V rows no column names, and the Q
    row of an empty row, are not used"""
    import torch
    tdt = _tdt(dtype)
    G = 8
    rp, ci, nrow = B.matrix()
    nnz = ci.size
    A, At = _handles(rp, ci, nrow, B.NCOL)
    for nk, nv in ((7, 5), (33, 129), (130, 16)):
        Q, K, V, dO, scale = B.operands(nk, nv, dtype, 5)
        Qd, Kd, Vd, dOd = _dev(gpu, Q, K, V, dO)
        Od, lsed = _forward(A, gpu, Qd, Kd, Vd, scale)
        clean = _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale)
        Qn, Kn, Vn = Q.copy(), K.copy(), V.copy()
        Qn[np.diff(rp) == 0] = np.nan
        unnamed = ~np.isin(np.arange(B.NCOL), ci)
        assert unnamed.any()
        Kn[unnamed] = np.nan
        Vn[unnamed] = np.nan
        Qd, Kd, Vd = _dev(gpu, Qn, Kn, Vn)
        for pad in (0, 3):
            def guarded(r, c):
                ld = c + pad
                flat = torch.full((G + r * ld + G,), SENT, dtype=tdt, device=gpu)
                return flat, torch.as_strided(flat, (r, c), (ld, 1), storage_offset=G)
            fQ, dQ = guarded(nrow, nk)
            fK, dK = guarded(B.NCOL, nk)
            fV, dV = guarded(B.NCOL, nv)
            dbuf = torch.full((nrow + 2 * G,), SENT, dtype=tdt, device=gpu)
            sbuf = torch.full((nnz + 2 * G,), SENT, dtype=tdt, device=gpu)
            A.attention_bwd_q(Qd, Kd, Vd, Od, dOd, lsed, scale=scale, dQ=dQ, delta=dbuf[G:G + nrow], ds_out=sbuf[G:G + nnz])
            At.attention_bwd_kv(Kd, Vd, Qd, dOd, lsed, dbuf[G:G + nrow], scale=scale, dK=dK, dV=dV)
            torch.cuda.synchronize()
            got = dict(dQ=dQ.cpu().numpy(), dK=dK.cpu().numpy(), dV=dV.cpu().numpy(), ds=sbuf[G:G + nnz].cpu().numpy(),
                       delta=dbuf[G:G + nrow].cpu().numpy())
            _same(clean, got, (dtype, nk, nv, pad, "unchanged by NaN in what no entry names"))
            for flat, r, c in ((fQ, nrow, nk), (fK, B.NCOL, nk), (fV, B.NCOL, nv)):
                f, ld = flat.cpu().numpy(), c + pad
                assert (f[:G] == SENT).all() and (f[G + (r - 1) * ld + c:] == SENT).all(), (dtype, nk, nv, pad, "guards")
                assert (f[G:G + (r - 1) * ld].reshape(r - 1, ld)[:, c:] == SENT).all(), (dtype, nk, nv, pad, "pad columns")
            db, sb = dbuf.cpu().numpy(), sbuf.cpu().numpy()
            assert (db[:G] == SENT).all() and (db[G + nrow:] == SENT).all() and (sb[:G] == SENT).all() and (sb[G + nnz:] == SENT).all()
    A.free()
    At.free()


def test_argument_errors_write_nothing(crp, gpu):
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    m, ncol = 500, 300
    rp, ci, va = gen.random_csr(m, ncol, 30, seed=3)
    nnz, nk, nv = ci.size, 16, 12
    A, At = _handles(rp, ci, m, ncol, va)
    codes = np.where(ci < 200, ci, ~(ci - 200)).astype(np.int32)
    A2 = hip.CsrDev(m, 200, rp, codes, va)
    for sfx, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        fq, fkv = getattr(lib, "crp_attention_bwd_q_csr_" + sfx), getattr(lib, "crp_attention_bwd_kv_csr_" + sfx)
        Q = torch.ones((m, nk), dtype=tdt, device=gpu)
        K = torch.ones((ncol, nk), dtype=tdt, device=gpu)
        V = torch.ones((ncol, nv), dtype=tdt, device=gpu)
        O = torch.ones((m, nv), dtype=tdt, device=gpu)
        lse = torch.zeros((m,), dtype=tdt, device=gpu)
        dlt = torch.zeros((m,), dtype=tdt, device=gpu)
        outs = [torch.full(s, SENT, dtype=tdt, device=gpu) for s in ((m, nk), (m,), (nnz,), (ncol, nk), (ncol, nv))]
        dQ, delta, ds, dK, dV = outs
        goodq = dict(A=A.handle, nk=nk, nv=nv, scale=1.0, bias=0, Q=Q.data_ptr(), ldQ=nk, K0=K.data_ptr(), ldK0=nk, K1=None, ldK1=0,
                     V0=V.data_ptr(), ldV0=nv, V1=None, ldV1=0, O=O.data_ptr(), ldO=nv, dO=O.data_ptr(), lddO=nv, lse=lse.data_ptr(),
                     dQ=dQ.data_ptr(), lddQ=nk, delta=delta.data_ptr(), ds_out=ds.data_ptr(), out_pos=None)
        goodkv = dict(A=At.handle, nk=nk, nv=nv, scale=1.0, bias=0, K=K.data_ptr(), ldK=nk, V=V.data_ptr(), ldV=nv, Q=Q.data_ptr(), ldQ=nk,
                      dO=O.data_ptr(), lddO=nv, lse=lse.data_ptr(), delta=dlt.data_ptr(), dK=dK.data_ptr(), lddK=nk, dV=dV.data_ptr(),
                      lddV=nv)

        def callq(**kw):
            a = dict(goodq, **kw)
            rc = fq(*[a[k] for k in ("A", "nk", "nv", "scale", "bias", "Q", "ldQ", "K0", "ldK0", "K1", "ldK1", "V0", "ldV0", "V1", "ldV1", "O",
                                     "ldO", "dO", "lddO", "lse", "dQ", "lddQ", "delta", "ds_out", "out_pos")], None)
            torch.cuda.synchronize()
            return rc

        def callkv(**kw):
            a = dict(goodkv, **kw)
            rc = fkv(*[a[k] for k in ("A", "nk", "nv", "scale", "bias", "K", "ldK", "V", "ldV", "Q", "ldQ", "dO", "lddO", "lse", "delta", "dK",
                                      "lddK", "dV", "lddV")], None)
            torch.cuda.synchronize()
            return rc
        cap = 512 if sfx == "f64" else 1024
        badq = [(dict(A=None), -1), (dict(Q=None), -1), (dict(O=None), -1), (dict(dO=None), -1), (dict(lse=None), -1), (dict(dQ=None), -1),
                (dict(delta=None), -1), (dict(K0=None), -1), (dict(V0=None), -1), (dict(nk=0), -1), (dict(nv=-2), -1), (dict(bias=2), -1),
                (dict(scale=float("inf")), -1), (dict(scale=float("nan")), -1), (dict(ldQ=nk - 1), -4), (dict(ldK0=nk - 1), -4),
                (dict(ldV0=nv - 1), -4), (dict(ldO=nv - 1), -4), (dict(lddO=nv - 1), -4), (dict(lddQ=nk - 1), -4),
                (dict(K1=K.data_ptr(), ldK1=nk - 1, V1=V.data_ptr(), ldV1=nv), -4), (dict(A=A2.handle), -1),
                (dict(nk=cap + 1, ldQ=cap + 1, ldK0=cap + 1, lddQ=cap + 1), B.EWIDTH),
                (dict(nv=cap + 1, ldV0=cap + 1, ldO=cap + 1, lddO=cap + 1), B.EWIDTH)]
        badkv = [(dict(A=None), -1), (dict(K=None), -1), (dict(V=None), -1), (dict(Q=None), -1), (dict(dO=None), -1), (dict(lse=None), -1),
                 (dict(delta=None), -1), (dict(dK=None), -1), (dict(dV=None), -1), (dict(nk=0), -1), (dict(nv=0), -1), (dict(bias=-1), -1),
                 (dict(scale=float("nan")), -1), (dict(A=A2.handle), -1), (dict(ldK=nk - 1), -4), (dict(ldV=nv - 1), -4),
                 (dict(ldQ=nk - 1), -4), (dict(lddO=nv - 1), -4), (dict(lddK=nk - 1), -4), (dict(lddV=nv - 1), -4),
                 (dict(nk=cap + 1, ldK=cap + 1, ldQ=cap + 1, lddK=cap + 1), B.EWIDTH),
                 (dict(nv=cap + 1, ldV=cap + 1, lddO=cap + 1, lddV=cap + 1), B.EWIDTH)]
        for call, bad in ((callq, badq), (callkv, badkv)):
            for kw, want in bad:
                rc = call(**kw)
                assert rc == want, (sfx, call.__name__, kw, rc)
                assert all(bool((t == SENT).all()) for t in outs), (sfx, call.__name__, kw, "something was written")
        assert callq() == 0 and callkv() == 0
        # K = V = O = dO = 1, lse = 0: dP = nv, delta = nv, dS = 0 exactly; p = exp(nk): dV[c] = (entries of column c) * exp(nk)
        assert bool((dQ == 0).all()) and bool((delta == nv).all()) and bool((ds == 0).all())
    A.free()
    At.free()
    A2.free()


def test_against_the_chain_of_existing_calls(crp, gpu):
    """the chain of tests/test_gpu_attention.py::test_one_backward_step_from_the_existing_calls on the same handles: the difference
    is at most the sum of the two bounds -- the fused backward's, and the chain's 8 c times the result formed from absolute values"""
    import torch
    from crp_spmm_amd import hip
    nk, nv, dtype = 33, 32, "float64"
    rp, ci, nrow, Q, K, V, dO, scale, ref = B.case(nk, nv, dtype)
    nnz = ci.size
    A, At = _handles(rp, ci, nrow, B.NCOL)
    Qd, Kd, Vd, dOd = _dev(gpu, Q, K, V, dO)
    Od, lsed = _forward(A, gpu, Qd, Kd, Vd, scale)
    got = _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale)
    p = torch.empty(nnz, dtype=torch.float64, device=gpu)
    A.attention(Qd, Kd, Vd, scale=scale, p_out=p)
    At.update_values(p)
    dV = torch.zeros((B.NCOL, nv), dtype=torch.float64, device=gpu)
    hip.spmm_csr(At, dOd, dV)
    dP = A.sddmm(dOd, Vd)
    dS = A.row_softmax_bwd(p, dP)
    A.update_values(dS)
    At.update_values(dS)
    dQ = torch.zeros((nrow, nk), dtype=torch.float64, device=gpu)
    dK = torch.zeros((B.NCOL, nk), dtype=torch.float64, device=gpu)
    hip.spmm_csr(A, Kd, dQ)
    hip.spmm_csr(At, Qd, dK)
    dQ.mul_(scale)
    dK.mul_(scale)
    torch.cuda.synchronize()
    c = 8 * 1.01 * R.coeff(ref["fwd"], dtype).max()
    mQ, mK, mV = B.chain_magnitudes(ref)
    for name, chain, mag, bound in (("dQ", dQ, mQ, B.bound_dQ), ("dK", dK, mK, B.bound_dK), ("dV", dV, mV, B.bound_dV)):
        tol = np.asarray(bound(ref, dtype) + c * mag)
        err = np.abs(got[name].astype(np.longdouble) - chain.cpu().numpy())
        print("%s: worst |fused - chain| / (sum of the bounds) = %.3g" % (name, float(B.worst(got[name].ravel(), chain.cpu().numpy().astype(np.longdouble).ravel(), tol.ravel())[0])))
        assert (err <= tol).all(), name
    A.free()
    At.free()


def test_sparse_attention_against_torch_autograd(crp, gpu):
    """hip.sparse_attention: gradients for Q, K and V through the two handles, against the reference (inside the bounds) and
    against torch autograd of the dense masked attention (the bound plus autograd's own 8 c share of the existing chain test)"""
    import torch
    from crp_spmm_amd import hip
    rp, ci, Q, K, V, dO, scale = B.dense_case()
    m = Q.shape[0]
    ref = B.reference(rp, ci, Q, K, V, dO, scale)
    A, At = _handles(rp, ci, m, m)
    Qd, Kd, Vd = (torch.from_numpy(x).to(gpu).requires_grad_(True) for x in (Q, K, V))
    O = hip.sparse_attention(A, At, Qd, Kd, Vd, scale=scale)
    O.backward(torch.from_numpy(dO).to(gpu))
    torch.cuda.synchronize()
    got = dict(dQ=Qd.grad.cpu().numpy(), dK=Kd.grad.cpu().numpy(), dV=Vd.grad.cpu().numpy())
    w = B.ratios(got, ref, "float64")
    print("sparse_attention: worst |grad - ref| / bound  %s" % w)
    assert all(v <= 1 for v in w.values()), w
    c = 8 * 1.01 * R.coeff(ref["fwd"], "float64").max()
    mags = dict(zip(("dQ", "dK", "dV"), B.chain_magnitudes(ref)))
    bounds = dict(dQ=B.bound_dQ, dK=B.bound_dK, dV=B.bound_dV)
    for key, want in zip(("dQ", "dK", "dV"), B.dense_autograd(rp, ci, Q, K, V, dO, scale)):
        assert (np.abs(got[key] - want) <= np.asarray(bounds[key](ref, "float64") + c * mags[key])).all(), key
    A.free()
    At.free()


def _engine_bwd(e, gpu, Qd, Kd, Vd, Od, dOd, lsed, scale, bias, nnz):
    import torch
    outs = [torch.full(s, float("nan"), dtype=Qd.dtype, device=gpu) for s in (tuple(Qd.shape), tuple(Kd.shape), tuple(Vd.shape), (nnz,))]
    dQ, dK, dV, ds = outs
    e.attention_bwd(Qd, Kd, Vd, Od, dOd, lsed, dQ, dK, dV, scale=scale, bias=bias, ds_out=ds)
    torch.cuda.synchronize()
    return dict(dQ=dQ.cpu().numpy(), dK=dK.cpu().numpy(), dV=dV.cpu().numpy(), ds=ds.cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_one_rank(crp, gpu, dtype):
    """RpSpmm.attention_bwd equals the handle calls bit for bit, timing on and off; the first call allocates (attention_bwd_built 0,
    then 1); the engine's values are unchanged (an exec before equals an exec after).  With bias the transposed matrices hold the
    engine's current values on every path that changes them.  First engine: update_values_dev BEFORE the transposed matrices
    exist -- the very first attention_bwd builds them from the downloaded device values (build_transposed after
    refresh_host_values) -- then a host update_values.  Second engine: a first exec_t builds them, then update_values_dev (the
    gather through dv_t_pos), then a host update_values (update_transposed_values)."""
    import torch
    from crp_spmm_amd import comm, engine, gen
    tdt = _tdt(dtype)
    sc = comm.SelfComm()
    m, k = 300, 260
    rp, ci, va = gen.random_csr(m, k, 40, empty_every=13)
    nnz = ci.size
    newv = np.random.default_rng(4).uniform(-3, 3, nnz)
    hostv = np.random.default_rng(6).uniform(-3, 3, nnz)
    DEV, HOST = "update_values_dev", "update_values"
    plans = ((24, False, ((DEV, True), (None, False), (HOST, True))),
             (65, True, ((None, False), (None, True), (DEV, True), (HOST, True))))
    for n, exec_t_first, steps in plans:
        A, At = _handles(rp, ci, m, k, va)
        e = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
        rng = np.random.default_rng(9)
        Q, K, V, Bm, dO = (rng.standard_normal(sh).astype(dtype) for sh in ((m, n), (k, n), (k, n), (k, n), (m, n)))
        Qd, Kd, Vd, Bd, dOd = _dev(gpu, Q, K, V, Bm, dO)
        scale = 1.0 / np.sqrt(n)
        C0 = torch.full((m, n), float("nan"), dtype=tdt, device=gpu)
        e.exec(0, Bd, C0)
        torch.cuda.synchronize()
        assert not e.attention_bwd_built()
        if exec_t_first:
            Ct = torch.full((k, n), float("nan"), dtype=tdt, device=gpu)
            (e.exec_t if dtype == "float64" else e.exec_t_f32)(0, dOd, Ct)
            torch.cuda.synchronize()
        assert e.transposed_built == exec_t_first
        for install, bias in steps:
            if install is not None:
                built = e.transposed_built
                if install == DEV:
                    vals = torch.from_numpy(newv).to(gpu)
                    e.update_values_dev(vals)
                else:
                    vals = hostv
                    e.update_values(vals)
                A.update_values(vals)
                At.update_values(vals)
                assert e.transposed_built == built          # a value update builds nothing
                e.exec(0, Bd, C0)
                torch.cuda.synchronize()
            Od, lsed = _forward(A, gpu, Qd, Kd, Vd, scale, bias=bias)
            want = _backward(A, At, gpu, Qd, Kd, Vd, Od, lsed, dOd, scale, bias=bias)
            assert all(np.isfinite(want[k_]).all() for k_ in KEYS)
            for timing in (True, False):
                e.set_timing(timing)
                got = _engine_bwd(e, gpu, Qd, Kd, Vd, Od, dOd, lsed, scale, bias, nnz)
                assert e.attention_bwd_built() and e.transposed_built
                _same(got, want, (dtype, n, install, bias, timing))
            C1 = torch.full((m, n), float("nan"), dtype=tdt, device=gpu)
            e.exec(0, Bd, C1)
            torch.cuda.synchronize()
            assert np.array_equal(C1.cpu().numpy(), C0.cpu().numpy()) and np.isfinite(C0.cpu().numpy()).all(), (dtype, n, install, "the engine's values")
        e.free()
        A.free()
        At.free()
    sc.free()


@pytest.mark.parametrize("world", [2, 4])
def test_multi_rank_one_gpu(world):
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    env.pop("CRPSPMM_EXPECT_NATIVE_RCCL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(30180 + world), os.path.join(ROOT, "tests", "gpu_dist_attention_bwd_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_ATTENTION_BWD_WORKER_OK world=%d" % world in r.stdout
