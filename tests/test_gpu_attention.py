"""GPU: the fused sparse attention over A's pattern (csrc/attention_kernels.hip, crp_attention_csr_f64 / _f32) and the
row-parallel engine's form.  Reference, bound (derived in DESIGN.md 5j) and data: tests/attention_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import attention_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
SENT = -77.0


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.array(a, order="C")).to(gpu) for a in arrays]


def _strided(gpu, a, ld, offset):
    """a copy of the 2-D array a on the device with leading dimension ld, starting `offset` elements into its allocation"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    flat = torch.full((a.shape[0] * ld + offset + 8,), float("nan"), dtype=t.dtype, device=gpu)
    view = torch.as_strided(flat, a.shape, (ld, 1), storage_offset=offset)
    view.copy_(t)
    return view


def _run(A, gpu, Q, K, V, scale, bias=False, K1=None, V1=None, nrow=None, want_lse=True, want_p=True, out_pos=None, p_out=None,
         out=None, lse=None):
    """one call -> (O, lse, p) as numpy arrays (None where not asked for)"""
    import torch
    nrow = Q.shape[0] if nrow is None else nrow
    if lse is None and want_lse:
        lse = torch.full((nrow,), float("nan"), dtype=Q.dtype, device=gpu)
    if p_out is None and want_p:
        p_out = torch.full((max(A.nnz, 1),), float("nan"), dtype=Q.dtype, device=gpu)[:A.nnz]
    O = A.attention(Q, K, V, K1=K1, V1=V1, scale=scale, bias=bias, out=out, lse=lse, p_out=p_out, out_pos=out_pos)
    torch.cuda.synchronize()
    return O.cpu().numpy(), None if lse is None else lse.cpu().numpy(), None if p_out is None else p_out.cpu().numpy()


def _check(got, ref, dtype, what):
    O, lse, p = got
    assert np.isfinite(O).all() and np.isfinite(p).all(), (what, "non-finite output")
    wo, ao = R.worst(O.ravel(), ref["O"].ravel(), R.bound_O(ref, dtype).ravel())
    wp, ap = R.worst(p, ref["p"], R.bound_p(ref, dtype))
    live = np.isfinite(ref["lse"].astype(np.float64))
    assert np.array_equal(np.isfinite(lse), live) and (lse[~live] == -np.inf).all(), (what, "lse of empty / masked rows")
    wl, al = R.worst(lse[live], ref["lse"][live], R.bound_lse(ref, dtype)[live])
    print("%s: worst |got - ref| / bound  O %.3g (at %d)  p_out %.3g (at %d)  lse %.3g (at %d)" % (what, wo, ao, wp, ap, wl, al))
    assert wo <= 1 and wp <= 1 and wl <= 1, (what, wo, wp, wl)
    return wo, wp, wl


@pytest.mark.parametrize("nk,nv,dtype", list(R.parity_cases()))
def test_parity(crp, gpu, nk, nv, dtype):
    """every instance threshold, nk != nv both ways, the V block path; rows of 0, 1, 7, 8, 9, 63, 64, 65, 200 and 5000 entries"""
    from crp_spmm_amd import hip
    rp, ci, Q, K, V, scale, ref = R.case(nk, nv, dtype)
    A = hip.CsrDev(R.NROW, R.NCOL, rp, ci, np.ones(ci.size))
    Qd, Kd, Vd = _dev(gpu, Q, K, V)
    got = _run(A, gpu, Qd, Kd, Vd, scale)
    _check(got, ref, dtype, ("parity", dtype, nk, nv, R.instance_of(nk, nv, dtype)))
    empty = np.diff(rp) == 0
    assert (got[0][empty] == 0).all() and not np.signbit(got[0][empty]).any()
    one = np.flatnonzero(np.diff(rp) == 1)
    assert np.array_equal(got[0][one], V[ci[rp[one]]]), "a one-entry row is its V row"
    A.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_sources_row_subsets_and_a_transposed_handle(crp, gpu, dtype):
    """parity inside the bound for each; the fixed-order test compares their bits"""
    import torch
    from crp_spmm_amd import hip
    nk, nv = 33, 17
    rp, ci, Q, K, V, scale, ref = R.case(nk, nv, dtype)
    Qd, Kd, Vd = _dev(gpu, Q, K, V)
    k0 = 2600
    codes = np.where(ci < k0, ci, ~(ci - k0)).astype(np.int32)
    A2 = hip.CsrDev(R.NROW, k0, rp, codes, np.ones(ci.size))
    _check(_run(A2, gpu, Qd, Kd[:k0], Vd[:k0], scale, K1=Kd[k0:], V1=Vd[k0:]), ref, dtype, ("two sources", dtype))
    A2.free()
    rows = R.rows_of(rp)
    pick = (np.arange(R.NROW) % 4) % 3 == 0
    O = torch.full((R.NROW, nv), float("nan"), dtype=_tdt(dtype), device=gpu)
    lse = torch.full((R.NROW,), float("nan"), dtype=_tdt(dtype), device=gpu)
    p = torch.full((ci.size,), float("nan"), dtype=_tdt(dtype), device=gpu)
    for sel in (pick, ~pick):
        r = np.flatnonzero(sel)
        keep = sel[rows]
        h = hip.CsrDev(r.size, R.NCOL, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], np.ones(int(keep.sum())))
        h.set_rowmap(r, R.NROW)
        pos = torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)
        h.attention(Qd, Kd, Vd, scale=scale, out=O, lse=lse, p_out=p, out_pos=pos)
        torch.cuda.synchronize()
        h.free()
    _check((O.cpu().numpy(), lse.cpu().numpy(), p.cpu().numpy()), ref, dtype, ("row subsets", dtype))
    # the transposed handle: A^T's rows are A's columns; its CSR order is (column, then row) of A
    order = np.lexsort((rows, ci))
    rpt = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=R.NCOL))]).astype(np.int32)
    cit = rows[order].astype(np.int32)
    rng = np.random.default_rng(3)
    Qt = rng.standard_normal((R.NCOL, nk)).astype(dtype)
    reft = R.reference(rpt, cit, Qt, K[:R.NROW], V[:R.NROW], scale)
    At = hip.CsrDev.from_transpose(R.NROW, R.NCOL, rp, ci, np.ones(ci.size))
    assert At.nrow == R.NCOL
    Qtd, = _dev(gpu, Qt)
    _check(_run(At, gpu, Qtd, Kd[:R.NROW], Vd[:R.NROW], scale), reft, dtype, ("transposed handle", dtype))
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_rescale_path(crp, gpu, dtype):
    """Rows led by a bias (the handle's values): ascending steeply, so that every batch raises the maximum; descending, so that
    none does; the maximum in the row's last (partial) batch; every second entry masked.  T up to 60."""
    from crp_spmm_amd import hip
    rp, ci, bias, Q, K, V, scale, ref = R.steep_case(dtype)
    A = hip.CsrDev(rp.size - 1, 80, rp, ci, bias)
    Qd, Kd, Vd = _dev(gpu, Q, K, V)
    got = _run(A, gpu, Qd, Kd, Vd, scale, bias=True)
    _check(got, ref, dtype, ("rescale rows", dtype))
    assert (got[2][~np.isfinite(bias)] == 0).all(), "masked entries of a mixed row"
    A.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases(crp, gpu, dtype):
    import torch
    from crp_spmm_amd import hip
    nk, nv = 17, 33
    rp, ci, Q, K, V, scale, ref = R.case(nk, nv, dtype)
    lens = np.diff(rp)
    rows = R.rows_of(rp)
    ne = np.flatnonzero(lens > 0)
    # Q = 0, integer V, rows of 2^k entries: every e is 1, l = 2^k, O the exact mean
    Vi = np.random.default_rng(1).integers(-50, 51, V.shape).astype(dtype)
    A = hip.CsrDev(R.NROW, R.NCOL, rp, ci, np.ones(ci.size))
    Kd, Vid, Vd, Qd = _dev(gpu, K, Vi, V, Q)
    O, lse, p = _run(A, gpu, torch.zeros_like(Qd), Kd, Vid, scale)
    pow2 = np.flatnonzero((lens > 0) & ((lens & (lens - 1)) == 0))
    assert {1, 2, 4, 8, 16, 32, 64} <= set(lens[pow2])
    sums = np.zeros((R.NROW, nv))
    sums[ne] = np.add.reduceat(Vi[ci].astype(np.float64), rp[ne], axis=0)
    dt = np.dtype(dtype)
    assert np.array_equal(O[ne], sums[ne].astype(dt) / lens[ne, None].astype(dt)), "the sum of integers over the length"
    assert np.array_equal(O[pow2], (sums[pow2] / lens[pow2, None]).astype(dt)), "the exact mean"
    assert np.array_equal(p, np.ones(ci.size, dt) / lens[rows].astype(dt))
    assert (p[np.isin(rows, pow2)] * lens[rows][np.isin(rows, pow2)] == 1).all()
    assert np.abs(lse[pow2] - np.log(lens[pow2].astype(np.longdouble))).max() <= 4 * R.U[dt] * np.log(64.0)
    # one-entry rows
    n1 = 300
    rp1 = np.arange(n1 + 1, dtype=np.int32)
    ci1 = np.random.default_rng(2).integers(0, R.NCOL, n1).astype(np.int32)
    A1 = hip.CsrDev(n1, R.NCOL, rp1, ci1, np.ones(n1))
    Q1, = _dev(gpu, np.random.default_rng(3).standard_normal((n1, nk)).astype(dtype))
    O1, lse1, p1 = _run(A1, gpu, Q1, Kd, Vd, scale)
    assert np.array_equal(O1, V[ci1]) and (p1 == 1).all() and np.isfinite(lse1).all()
    A1.free()
    # masks: every row of 3 | r fully masked, every fifth entry of the other rows masked
    bias = np.zeros(ci.size)
    bias[np.arange(ci.size) % 5 == 0] = -np.inf
    bias[rows % 3 == 0] = -np.inf
    A.update_values(bias)
    O, lse, p = _run(A, gpu, Qd, Kd, Vd, scale, bias=True)
    refm = R.reference(rp, ci, Q, K, V, scale, bias.astype(dtype))
    _check((O, lse, p), refm, dtype, ("masked", dtype))
    dead = (lens == 0) | (np.arange(R.NROW) % 3 == 0) | (np.bincount(rows[np.isfinite(bias)], minlength=R.NROW) == 0)
    assert (O[dead] == 0).all() and (lse[dead] == -np.inf).all(), "empty and all-masked rows"
    assert (p[~np.isfinite(bias)] == 0).all(), "masked entries"
    # the rows of p_out sum to 1 inside the bound
    tot = np.zeros(R.NROW, np.longdouble)
    tot[ne] = np.add.reduceat(p.astype(np.longdouble), rp[ne])
    live = ~dead
    assert (np.abs(tot[live] - 1) <= 1.01 * R.coeff(refm, dtype)[live]).all()
    assert (tot[dead] == 0).all()
    A.free()


FIXED = {"float64": ((3, 3), (16, 16), (33, 33), (8, 40), (130, 4), (129, 129), (520, 520), (4, 1030)),
         "float32": ((3, 3), (16, 16), (33, 33), (8, 40), (130, 4), (129, 129), (520, 520), (8, 2100))}


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_order(crp, gpu, dtype):
    """Bit-identical: two calls; operands one element off and at odd leading dimensions against aligned ones; one source against
    two; the full handle against two row subsets; with and without lse / p_out."""
    import torch
    from crp_spmm_amd import hip
    rp, ci = R.matrix()
    rows = R.rows_of(rp)
    nnz = ci.size
    val = np.random.default_rng(8).uniform(-2, 2, nnz)
    A = hip.CsrDev(R.NROW, R.NCOL, rp, ci, val)
    k0 = 2600
    codes = np.where(ci < k0, ci, ~(ci - k0)).astype(np.int32)
    A2 = hip.CsrDev(R.NROW, k0, rp, codes, val)
    pick = (np.arange(R.NROW) % 4) % 3 == 0
    subs = []
    for sel in (pick, ~pick):
        r = np.flatnonzero(sel)
        keep = sel[rows]
        h = hip.CsrDev(r.size, R.NCOL, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], val[keep])
        h.set_rowmap(r, R.NROW)
        subs.append((h, torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)))
    tdt = _tdt(dtype)
    for nk, nv in FIXED[dtype]:
        Q, K, V, scale = R.operands(nk, nv, dtype, 9000 + nk + nv)
        Qd, Kd, Vd = _dev(gpu, Q, K, V)
        for bias in (False, True):
            what = (dtype, nk, nv, bias)
            base = _run(A, gpu, Qd, Kd, Vd, scale, bias=bias)
            assert np.isfinite(base[0]).all() and np.isfinite(base[2]).all(), what
            again = _run(A, gpu, Qd, Kd, Vd, scale, bias=bias)
            assert all(np.array_equal(a, b) for a, b in zip(again, base)), (what, "two consecutive calls")
            bare = _run(A, gpu, Qd, Kd, Vd, scale, bias=bias, want_lse=False, want_p=False)
            assert np.array_equal(bare[0], base[0]), (what, "without lse and p_out")
            only_p = _run(A, gpu, Qd, Kd, Vd, scale, bias=bias, want_lse=False)
            assert np.array_equal(only_p[0], base[0]) and np.array_equal(only_p[2], base[2]), (what, "without lse")
            # pointers one element into their allocations, odd leading dimensions; the output too
            out = _strided(gpu, np.zeros((R.NROW, nv), dtype), nv + 1, 1)
            got = _run(A, gpu, _strided(gpu, Q, nk + 1, 1), _strided(gpu, K, nk + 3, 1), _strided(gpu, V, nv + 1, 3), scale, bias=bias, out=out)
            assert all(np.array_equal(a, b) for a, b in zip(got, base)), (what, "offset pointers, odd leading dimensions")
            got = _run(A, gpu, Qd, _strided(gpu, K, nk + 5, 0), Vd, scale, bias=bias)
            got2 = _run(A, gpu, _strided(gpu, Q, nk, 1), Kd, _strided(gpu, V, nv + 2, 0), scale, bias=bias)
            assert all(np.array_equal(a, b) for a, b in zip(got, base)) and all(np.array_equal(a, b) for a, b in zip(got2, base)), \
                (what, "mixed alignment")
            got = _run(A2, gpu, Qd, Kd[:k0], Vd[:k0], scale, bias=bias, K1=_strided(gpu, K[k0:], nk + 4, 0), V1=_strided(gpu, V[k0:], nv + 4, 0))
            got2 = _run(A2, gpu, Qd, Kd[:k0], Vd[:k0], scale, bias=bias, K1=_strided(gpu, K[k0:], nk + 5, 3), V1=Vd[k0:])
            assert all(np.array_equal(a, b) for a, b in zip(got, base)) and all(np.array_equal(a, b) for a, b in zip(got2, base)), \
                (what, "two sources")
            O = torch.full((R.NROW, nv), SENT, dtype=tdt, device=gpu)
            lse = torch.full((R.NROW,), SENT, dtype=tdt, device=gpu)
            p = torch.full((nnz,), SENT, dtype=tdt, device=gpu)
            h, pos = subs[0]
            half = _run(h, gpu, Qd, Kd, Vd, scale, bias=bias, out=O, lse=lse, p_out=p, out_pos=pos)
            named = np.zeros(nnz, bool)
            named[pos.cpu().numpy()] = True
            assert np.array_equal(half[0][pick], base[0][pick]) and (half[0][~pick] == SENT).all(), (what, "first subset, O")
            assert np.array_equal(half[1][pick], base[1][pick]) and (half[1][~pick] == SENT).all(), (what, "first subset, lse")
            assert np.array_equal(half[2][named], base[2][named]) and (half[2][~named] == SENT).all(), (what, "first subset, p_out")
            h, pos = subs[1]
            full = _run(h, gpu, Qd, Kd, Vd, scale, bias=bias, out=O, lse=lse, p_out=p, out_pos=pos)
            assert all(np.array_equal(a, b) for a, b in zip(full, base)), (what, "row subsets")
    for h in [A, A2] + [s[0] for s in subs]:
        h.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_chain_and_the_sddmm_scores(crp, gpu, dtype):
    """O within the sum of the two bounds of sddmm -> scale -> row_softmax -> update_values -> product on the same handle; and with
    scale = 1, lse and p_out are those of scores that equal the SDDMM's bits (the exact softmax of the SDDMM's output, the
    bound without its score term)."""
    import torch
    from crp_spmm_amd import hip
    u = R.U[np.dtype(dtype)]
    for nk, nv in ((16, 16), (65, 33)):
        rp, ci, Q, K, V, scale, ref = R.case(nk, nv, dtype)
        rows = R.rows_of(rp)
        A = hip.CsrDev(R.NROW, R.NCOL, rp, ci, np.ones(ci.size))
        Qd, Kd, Vd = _dev(gpu, Q, K, V)
        fused = _run(A, gpu, Qd, Kd, Vd, scale)
        s = A.sddmm(Qd, Kd)
        s.mul_(scale)
        y = A.row_softmax(s)
        A.update_values(y.double())
        Cd = torch.zeros((R.NROW, nv), dtype=_tdt(dtype), device=gpu)
        (hip.spmm_csr if dtype == "float64" else hip.spmm_csr_f32)(A, Vd, Cd)
        torch.cuda.synchronize()
        chain = Cd.cpu().numpy()
        # the chain's own bound: the scores (nk + 2) u |scale| S shift the exponents, the softmax (L + 2 T + 8) u (tests/softmax_ref.py),
        # the product of L terms (L + 2) u, the fp32 product's copy of the value one more
        L, T, D = ref["L"], ref["T"], ref["D"].astype(np.float64) * (nk + 2) / (nk + 1)
        c_chain = 1.01 * ((2 * L + 2 * T + 11) + 2 * D) * u
        both = R.bound_O(ref, dtype) + c_chain[:, None] * ref["A"]
        err = np.abs(fused[0].astype(np.longdouble) - chain.astype(np.longdouble))
        w, at = R.worst(fused[0].ravel(), chain.astype(np.longdouble).ravel(), both.ravel())
        print("fused against the chain %s nk=%d nv=%d: worst |diff| / (bound + bound) = %.3g" % (dtype, nk, nv, w))
        assert (err <= both).all(), (dtype, nk, nv, w, at)
        # scale = 1: the scores are the SDDMM's bits
        A.update_values(np.ones(ci.size))
        s1 = A.sddmm(Qd, Kd)
        got = _run(A, gpu, Qd, Kd, Vd, 1.0)
        torch.cuda.synchronize()
        sl = s1.cpu().numpy().astype(np.longdouble)
        ne = np.flatnonzero(np.diff(rp) > 0)
        m = np.full(R.NROW, -np.inf, np.longdouble)
        m[ne] = np.maximum.reduceat(sl, rp[ne])
        e = np.exp(sl - m[rows])
        tot = np.zeros(R.NROW, np.longdouble)
        tot[ne] = np.add.reduceat(e, rp[ne])
        T1 = np.zeros(R.NROW)
        T1[ne] = np.maximum.reduceat((m[rows] - sl).astype(np.float64), rp[ne])
        assert T1.max() <= 60
        c1 = 1.01 * (2 * L + 4 * T1 + 10 * np.ceil(L / 8) + 9) * u
        pref = e / tot[rows]
        assert (np.abs(got[2] - pref) <= c1[rows] * pref).all(), (dtype, nk, nv, "p_out against the softmax of the SDDMM's scores")
        lref = m[ne] + np.log(tot[ne])
        bl = c1[ne] + 1.01 * u * (4 * np.abs(np.log(tot[ne])) + np.abs(m[ne]) + np.abs(lref)).astype(np.float64)
        assert (np.abs(got[1][ne] - lref) <= bl).all(), (dtype, nk, nv, "lse against the SDDMM's scores")
        A.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_only_what_is_named_is_touched(crp, gpu, dtype):
    """guard bands around O, lse and p_out and the pad columns of O keep their sentinel; K / V rows no column names and the Q row
    of an empty row are not used"""
    import torch
    from crp_spmm_amd import hip
    tdt = _tdt(dtype)
    G = 8
    for nk, nv in ((7, 5), (33, 129), (130, 16)):
        rp, ci, Q, K, V, scale, ref = R.case(33, 33, dtype)[:2] + R.operands(nk, nv, dtype, 5) + (None,)
        nnz = ci.size
        A = hip.CsrDev(R.NROW, R.NCOL, rp, ci, np.ones(nnz))
        Qd, Kd, Vd = _dev(gpu, Q, K, V)
        clean = _run(A, gpu, Qd, Kd, Vd, scale)
        Qn, Kn, Vn = Q.copy(), K.copy(), V.copy()
        Qn[np.diff(rp) == 0] = np.nan
        unnamed = ~np.isin(np.arange(R.NCOL), ci)
        assert unnamed.sum() > 50
        Kn[unnamed] = np.nan
        Vn[unnamed] = np.nan
        Qd, Kd, Vd = _dev(gpu, Qn, Kn, Vn)
        for ld in (nv, nv + 3):
            flat = torch.full((G + R.NROW * ld + G,), SENT, dtype=tdt, device=gpu)
            O = torch.as_strided(flat, (R.NROW, nv), (ld, 1), storage_offset=G)
            lbuf = torch.full((R.NROW + 2 * G,), SENT, dtype=tdt, device=gpu)
            pbuf = torch.full((nnz + 2 * G,), SENT, dtype=tdt, device=gpu)
            got = _run(A, gpu, Qd, Kd, Vd, scale, out=O, lse=lbuf[G:G + R.NROW], p_out=pbuf[G:G + nnz])
            assert all(np.array_equal(a, b) for a, b in zip(got, clean)), (dtype, nk, nv, ld, "unchanged by NaN in what no entry names")
            f = flat.cpu().numpy()
            assert (f[:G] == SENT).all() and (f[G + (R.NROW - 1) * ld + nv:] == SENT).all(), (dtype, nk, nv, ld, "guards of O")
            body = f[G:G + (R.NROW - 1) * ld].reshape(R.NROW - 1, ld)
            assert (body[:, nv:] == SENT).all(), (dtype, nk, nv, ld, "pad columns of O")
            lb, pb = lbuf.cpu().numpy(), pbuf.cpu().numpy()
            assert (lb[:G] == SENT).all() and (lb[G + R.NROW:] == SENT).all() and (pb[:G] == SENT).all() and (pb[G + nnz:] == SENT).all()
        A.free()


def test_argument_errors_write_nothing(crp, gpu):
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    rp, ci, va = gen.random_csr(500, 300, 30, seed=3)
    nnz, nk, nv = ci.size, 16, 12
    A = hip.CsrDev(500, 300, rp, ci, va)
    codes = np.where(ci < 200, ci, ~(ci - 200)).astype(np.int32)
    A2 = hip.CsrDev(500, 200, rp, codes, va)
    for fn, tdt in ((lib.crp_attention_csr_f64, torch.float64), (lib.crp_attention_csr_f32, torch.float32)):
        Q = torch.ones((500, nk), dtype=tdt, device=gpu)
        K = torch.ones((300, nk), dtype=tdt, device=gpu)
        V = torch.ones((300, nv), dtype=tdt, device=gpu)
        O = torch.full((500, nv), SENT, dtype=tdt, device=gpu)
        lse = torch.full((500,), SENT, dtype=tdt, device=gpu)
        p = torch.full((nnz,), SENT, dtype=tdt, device=gpu)
        good = dict(A=A.handle, nk=nk, nv=nv, scale=1.0, bias=0, Q=Q.data_ptr(), ldQ=nk, K0=K.data_ptr(), ldK0=nk, K1=None, ldK1=0,
                    V0=V.data_ptr(), ldV0=nv, V1=None, ldV1=0, O=O.data_ptr(), ldO=nv, lse=lse.data_ptr(), p_out=p.data_ptr(), out_pos=None)

        def call(**kw):
            a = dict(good, **kw)
            rc = fn(a["A"], a["nk"], a["nv"], a["scale"], a["bias"], a["Q"], a["ldQ"], a["K0"], a["ldK0"], a["K1"], a["ldK1"], a["V0"],
                    a["ldV0"], a["V1"], a["ldV1"], a["O"], a["ldO"], a["lse"], a["p_out"], a["out_pos"], None)
            torch.cuda.synchronize()
            return rc
        bad = [(dict(A=None), -1), (dict(Q=None), -1), (dict(O=None), -1), (dict(K0=None), -1), (dict(V0=None), -1), (dict(nk=0), -1),
               (dict(nv=0), -1), (dict(nk=-3), -1), (dict(bias=2), -1), (dict(bias=-1), -1), (dict(scale=float("inf")), -1),
               (dict(scale=float("nan")), -1), (dict(ldQ=nk - 1), -4), (dict(ldK0=nk - 1), -4), (dict(ldV0=nv - 1), -4), (dict(ldO=nv - 1), -4),
               (dict(K1=K.data_ptr(), ldK1=nk - 1, V1=V.data_ptr(), ldV1=nv), -4), (dict(K1=K.data_ptr(), ldK1=nk, V1=V.data_ptr(), ldV1=nv - 1), -4),
               (dict(A=A2.handle), -1), (dict(A=A2.handle, K1=K.data_ptr(), ldK1=nk), -1)]      # negative codes and no second source
        for kw, want in bad:
            rc = call(**kw)
            assert rc == want, (fn.__name__, kw, rc)
            assert bool((O == SENT).all()) and bool((lse == SENT).all()) and bool((p == SENT).all()), (fn.__name__, kw, "something was written")
        assert call() == 0
        # K = 1, V = 1: the scores of a row are equal, every e is 1 and O = L / L
        lens = torch.from_numpy(np.diff(rp)).to(gpu)
        assert bool((O[lens > 0] == 1).all()) and bool((O[lens == 0] == 0).all())
        assert bool((p * lens[torch.from_numpy(R.rows_of(rp)).to(gpu)] - 1).abs().max() <= 2.0 ** -22)
    A.free()
    A2.free()


def test_one_backward_step_from_the_existing_calls(crp, gpu):
    """p_out -> dV by the transposed product, dP by sddmm(dO, V), dS by row_softmax_bwd, dQ and dK by the products with values dS,
    against torch autograd on the dense masked attention in fp64.  Tolerance: each of the four steps and each of the two
    computations errs by at most c (the forward's coefficient, tests/attention_ref.py, which exceeds every step's own) times the
    step's result formed from absolute values, hence 8 c times that."""
    import torch
    from crp_spmm_amd import hip
    m, nk, nv = 64, 16, 24
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 13, m)                                   # (no empty row: torch's softmax of one is NaN)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(m, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    rows = R.rows_of(rp)
    nnz = ci.size
    Q, K, V, scale = R.operands(nk, nv, "float64", 21, nrow=m, ncol=m)
    dO = np.random.default_rng(22).standard_normal((m, nv))
    A = hip.CsrDev(m, m, rp, ci, np.ones(nnz))
    At = hip.CsrDev.from_transpose(m, m, rp, ci, np.ones(nnz))
    Qd, Kd, Vd, dOd = _dev(gpu, Q, K, V, dO)
    p = torch.empty(nnz, dtype=torch.float64, device=gpu)
    A.attention(Qd, Kd, Vd, scale=scale, p_out=p)
    At.update_values(p)
    dV = torch.zeros((m, nv), dtype=torch.float64, device=gpu)
    hip.spmm_csr(At, dOd, dV)
    dP = A.sddmm(dOd, Vd)
    dS = A.row_softmax_bwd(p, dP)
    A.update_values(dS)
    At.update_values(dS)
    dQ = torch.zeros((m, nk), dtype=torch.float64, device=gpu)
    dK = torch.zeros((m, nk), dtype=torch.float64, device=gpu)
    hip.spmm_csr(A, Kd, dQ)
    hip.spmm_csr(At, Qd, dK)
    dQ.mul_(scale)
    dK.mul_(scale)
    torch.cuda.synchronize()
    # autograd on the dense masked attention
    Qt, Kt, Vt = (torch.from_numpy(x).clone().requires_grad_(True) for x in (Q, K, V))
    mask = torch.zeros((m, m), dtype=torch.bool)
    mask[torch.from_numpy(rows), torch.from_numpy(ci.astype(np.int64))] = True
    S = (Qt @ Kt.T) * scale
    P = torch.softmax(S.masked_fill(~mask, float("-inf")), dim=1)
    P = torch.where(mask.any(dim=1, keepdim=True), P, torch.zeros_like(P))
    (P @ Vt).backward(torch.from_numpy(dO))
    ref = R.reference(rp, ci, Q, K, V, scale)
    c = 8 * 1.01 * R.coeff(ref, "float64").max()
    Pd = P.detach().numpy()
    aP = np.abs(dO) @ np.abs(V).T                                   # |dP| <= sum_j |dO_ij| |V_cj|
    aS = Pd * (aP + (Pd * aP).sum(axis=1, keepdims=True))           # |dS| <= p (|dP| + sum_q p_q |dP_q|)
    for name, got, want, mag in (("dV", dV, Vt.grad, Pd.T @ np.abs(dO)), ("dQ", dQ, Qt.grad, abs(scale) * (aS @ np.abs(K))),
                                 ("dK", dK, Kt.grad, abs(scale) * (aS.T @ np.abs(Q)))):
        err = np.abs(got.cpu().numpy() - want.numpy())
        with np.errstate(divide="ignore", invalid="ignore"):
            print("%s: worst |got - autograd| / (8 c magnitude) = %.3g" % (name, float(np.nanmax(np.where(mag > 0, err / (c * mag), 0)))))
        assert (err <= c * mag).all(), name
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_one_rank(crp, gpu, dtype):
    """RpSpmm.attention equals the device-level call bit for bit with device and host operands in both layouts; the first call
    allocates (attention_built 0, then 1); values installed by update_values_dev act as the bias; the engine's values are
    unchanged: an exec before equals an exec after."""
    import torch
    from crp_spmm_amd import comm, engine, gen, hip
    tdt = _tdt(dtype)
    sc = comm.SelfComm()
    rp, ci, va = gen.random_csr(300, 260, 40, empty_every=13)
    m, k, nnz = 300, 260, ci.size
    for n in (24, 65):
        A = hip.CsrDev(m, k, rp, ci, va)
        e = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
        rng = np.random.default_rng(9)
        Q, K, V, B = (rng.standard_normal(sh).astype(dtype) for sh in ((m, n), (k, n), (k, n), (k, n)))
        Qd, Kd, Vd, Bd = _dev(gpu, Q, K, V, B)
        scale = 1.0 / np.sqrt(n)
        C0 = torch.full((m, n), float("nan"), dtype=tdt, device=gpu)
        e.exec(0, Bd, C0)
        torch.cuda.synchronize()
        assert not e.attention_built()
        newv = torch.from_numpy(np.random.default_rng(4).uniform(-3, 3, nnz)).to(gpu)
        for bias in (False, True, "installed"):
            if bias == "installed":
                e.update_values_dev(newv)
                A.update_values(newv)
                e.exec(0, Bd, C0)
                torch.cuda.synchronize()
            want = _run(A, gpu, Qd, Kd, Vd, scale, bias=bool(bias))
            for timing in (True, False):
                e.set_timing(timing)
                O = torch.full((m, n), float("nan"), dtype=tdt, device=gpu)
                lse = torch.full((m,), float("nan"), dtype=tdt, device=gpu)
                p = torch.full((nnz,), float("nan"), dtype=tdt, device=gpu)
                e.attention(0, Qd, Kd, Vd, O, scale=scale, bias=bool(bias), lse=lse, p_out=p)
                torch.cuda.synchronize()
                assert e.attention_built()
                got = (O.cpu().numpy(), lse.cpu().numpy(), p.cpu().numpy())
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (dtype, n, bias, timing, "device operands")
                O.fill_(float("nan"))
                Ot = torch.full((n, m), float("nan"), dtype=tdt, device=gpu)
                e.attention(1, Qd.t().contiguous(), Kd.t().contiguous(), Vd.t().contiguous(), Ot, scale=scale, bias=bool(bias))
                torch.cuda.synchronize()
                assert np.array_equal(Ot.t().cpu().numpy(), want[0]), (dtype, n, bias, timing, "device operands, column-major")
                Oh, lh, ph = np.full((m, n), np.nan, dtype), np.full(m, np.nan, dtype), np.full(nnz, np.nan, dtype)
                e.attention(0, Q, K, V, Oh, scale=scale, bias=bool(bias), lse=lh, p_out=ph)
                assert all(np.array_equal(a, b) for a, b in zip((Oh, lh, ph), want)), (dtype, n, bias, timing, "host operands")
                Oh = np.full((n, m), np.nan, dtype)
                e.attention(1, np.ascontiguousarray(Q.T), np.ascontiguousarray(K.T), np.ascontiguousarray(V.T), Oh, scale=scale,
                            bias=bool(bias), p_out=ph)
                assert np.array_equal(Oh.T, want[0]) and np.array_equal(ph, want[2]), (dtype, n, bias, timing, "host operands, column-major")
            C1 = torch.full((m, n), float("nan"), dtype=tdt, device=gpu)
            e.exec(0, Bd, C1)
            torch.cuda.synchronize()
            assert np.array_equal(C1.cpu().numpy(), C0.cpu().numpy()) and np.isfinite(C0.cpu().numpy()).all(), (dtype, n, bias, "the engine's values")
        e.free()
        A.free()
    sc.free()


@pytest.mark.parametrize("world", [2, 4])
def test_multi_rank_one_gpu(world):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    env.pop("CRPSPMM_EXPECT_NATIVE_RCCL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(30140 + world), os.path.join(ROOT, "tests", "gpu_dist_attention_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_ATTENTION_WORKER_OK world=%d" % world in r.stdout
