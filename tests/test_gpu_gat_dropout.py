"""GPU: attention dropout in the fused GAT attention and its two-handle backward (crp_gat_attention_drop_csr_*, _bwd_row_, _bwd_col_,
crp_dropout_mask_csr, the CsrDev keywords and hip.gat_attention(dropout=, seed=)).

The mask against numpy's Philox entry for entry, over A, over A^T and over a row-subset pair.  dropout = 0 against the existing
calls, bit for bit.  Exact pins against the kernels that exist (torch.equal, nothing compared with the code under test): with
V = I every column of O holds one entry's term, so O_drop == where(k, fl(O_plain rs), +0); lse and p_out are the plain call's; with
dO = I on the column side dV_drop == where(k, fl(dV_plain rs), +0); and on a matrix with one entry per column and slope = 1 the
row side's ds_out is the column side's d_er.  Then everything inside the bound of DESIGN.md 5q against
tests/dropout_ref.gat_reference, the invariances, the special cases and hip.gat_attention against torch autograd.

Head h of an H-head call is NOT the one-head call on head h's views under dropout: the key of the draw holds h.  That invariance
of 5n is not claimed here (and test_invariance shows the two masks differ)."""
import numpy as np
import pytest

import attention_bwd_ref as B
import attention_ref as R
import dropout_ref as D
import gat_ref as G
from test_gpu_attention import SENT, _strided, _tdt
from test_gpu_gat import _dev, _handles, _nan, _same

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
KEYS = G.FWD_KEYS + G.BWD_KEYS


def _gat(A, At, gpu, el, er, V, dO, H, slope, drop, seed, bias=False, er1=None, V1=None, backward=True):
    """one forward, row side and (At given) column side under dropout -> dict of device tensors, every output asked for"""
    import torch
    nrow, nnz = el.shape[0], A.nnz
    kw = dict(slope=slope, bias=bias, heads=H, dropout=drop, seed=seed)
    lse, p = _nan(gpu, V, nrow, H), _nan(gpu, V, nnz, H)
    O = A.gat_attention(el, er, V, er1=er1, V1=V1, lse=lse, p_out=p, **kw)
    out = dict(O=O, lse=lse, p=p)
    if backward:
        ds = _nan(gpu, V, nnz, H)
        d_el, delta = A.gat_attention_bwd_row(el, er, V, O, dO, lse, er1=er1, V1=V1, ds_out=ds, **kw)
        out.update(delta=delta, ds=ds, d_el=d_el)
        if At is not None:
            d_er, dV = At.gat_attention_bwd_col(er, V, el, dO, lse, delta, **kw)
            out.update(d_er=d_er, dV=dV)
    torch.cuda.synchronize()
    return out


def _ratios(got, ref, what):
    r = D.ratios({k: v.cpu().numpy() for k, v in got.items()}, ref)
    print("%s: worst |got - ref| / bound  %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) <= 1, (what, r)
    return r


# ---- the mask ---------------------------------------------------------------------------------------------------------

def test_dropout_mask_is_numpys(crp, gpu):
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.matrix()
    nrow, ncol, nnz = G.NROW, G.NCOL, ci.size
    A, At = _handles(rp, ci, nrow, ncol)
    rpt, cit, tmap = B.transpose(rp, ci, ncol)
    assert At.is_transposed and not A.is_transposed
    for H in (1, 3):
        for drop, seed in ((D.DROP, D.SEED), (0.6, 7), (0.1, (1 << 64) - 1), (0.0, 5), (2.0 ** -33, 5)):
            want = D.mask_csr(rp, ci, H, drop, seed)
            m = A.dropout_mask(H, drop, seed)
            mt = At.dropout_mask(H, drop, seed)
            torch.cuda.synchronize()
            assert m.dtype == torch.uint8 and tuple(m.shape) == (nnz, H)
            assert np.array_equal(m.cpu().numpy(), want.astype(np.uint8)), (H, drop, "over A")
            assert np.array_equal(mt.cpu().numpy(), want[tmap].astype(np.uint8)), (H, drop, "over A^T: the same bits, transposed")
            if drop < 2.0 ** -32:
                assert want.all()
    # two sources: the code goes in as its bit pattern
    codes = G.two_source_codes(ci)
    A2 = hip.CsrDev(nrow, G.K0, rp, codes, np.ones(nnz))
    got = A2.dropout_mask(3, D.DROP, D.SEED).cpu().numpy()
    want2 = D.mask_csr(rp, codes, 3, D.DROP, D.SEED)
    assert np.array_equal(got, want2.astype(np.uint8)) and (want2 != D.mask_csr(rp, ci, 3, D.DROP, D.SEED)).any()
    A2.free()
    # a row-subset pair with row maps and out_pos (a permutation of the full positions) reproduces the full matrix's flags
    H = 3
    want = D.mask_csr(rp, ci, H, D.DROP, D.SEED)
    rows = R.rows_of(rp)
    perm = np.random.default_rng(2).permutation(nnz).astype(np.int32)
    out = torch.full((nnz + 1, H), 9, dtype=torch.uint8, device=gpu)
    pick = (np.arange(nrow) % 4) % 3 == 0
    for sel in (pick, ~pick):
        r = np.flatnonzero(sel)
        keep = sel[rows]
        h = hip.CsrDev(r.size, ncol, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], np.ones(int(keep.sum())))
        h.set_rowmap(r, nrow)
        pos = torch.from_numpy(perm[np.flatnonzero(keep)]).to(gpu)
        assert h.dropout_mask(H, D.DROP, D.SEED, out=out, out_pos=pos) is out
        torch.cuda.synchronize()
        h.free()
    got = out.cpu().numpy()
    assert np.array_equal(got[:nnz][perm], want.astype(np.uint8)) and (got[nnz] == 9).all()
    A.free()
    At.free()


# ---- dropout = 0 and the exact pins -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_zero_is_the_existing_call(crp, gpu, dtype):
    from test_gpu_gat import _gat as plain
    rp, ci = G.matrix()
    val = np.random.default_rng(8).standard_normal(ci.size)
    A, At = _handles(rp, ci, G.NROW, G.NCOL, val)
    for i, dv in enumerate(G.widths(dtype)):
        H = (1, 3)[i % 2]
        el, er, V, dO = _dev(gpu, *G.operands(dtype, H, dv, 2.0, 40 + i))
        want = plain(A, At, gpu, el, er, V, dO, H, 0.2, bias=True)
        _same(_gat(A, At, gpu, el, er, V, dO, H, 0.2, 0.0, D.SEED, bias=True), want, (dtype, H, dv, "dropout = 0"))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_with_identity_values_and_lse_and_p_out(crp, gpu, dtype):
    """V = I (dv = the number of columns): O_drop == where(k, fl(O_plain rs), +0) bit for bit, on the 40 x 80 matrix and on an
    8-column one (the group of 8 lanes); lse and p_out are the existing call's at any rate"""
    import torch
    from test_gpu_gat import _gat as plain
    dt = np.dtype(dtype)
    for (rp, ci, ncol), H in (((*G.matrix(), G.NCOL), 1), ((*G.matrix(), G.NCOL), 3), (D.narrow_matrix(), 1), (D.narrow_matrix(), 3)):
        nrow = rp.size - 1
        A, _ = _handles(rp, ci, nrow, ncol)
        el, er, _, _ = G.operands(dtype, H, 1, 2.0, 33, nrow=nrow, ncol=ncol)
        Vn = np.tile(np.eye(ncol, dtype=dt), (1, H))
        el, er, V = _dev(gpu, el, er, Vn)
        want = plain(A, None, gpu, el, er, V, None, H, 0.2, backward=False)
        On = want["O"].cpu().numpy()
        for drop in (D.PIN_DROP, D.DROP, 0.9):
            rs = D.rs_of(drop, dt)
            k = D.mask_csr(rp, ci, H, drop, D.SEED)
            got = _gat(A, None, gpu, el, er, V, None, H, 0.2, drop, D.SEED, backward=False)
            _same(got, want, (dtype, H, ncol, drop, "lse and p_out"), keys=("lse", "p"))
            for h in range(H):
                sv = slice(h * ncol, (h + 1) * ncol)
                K = D.dense_mask(rp, ci, ncol, k[:, h])
                exp = np.where(K, (On[:, sv] * rs).astype(dt), dt.type(0))
                mine = got["O"][:, sv].cpu().numpy()
                assert np.array_equal(mine, exp) and not np.signbit(mine[~K]).any(), (dtype, H, ncol, drop, h)
            assert (k == 0).any() and (k == 1).any()
        A.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_side_with_identity_gradient(crp, gpu, dtype):
    """dO rows as unit vectors (dv = the number of rows): dV_drop == where(k, fl(dV_plain rs), +0) bit for bit"""
    from test_gpu_gat import _gat as plain
    dt = np.dtype(dtype)
    rp, ci = G.matrix()
    nrow, ncol = G.NROW, G.NCOL
    A, At = _handles(rp, ci, nrow, ncol)
    for H in (1, 3):
        el, er, V, _ = G.operands(dtype, H, nrow, 2.0, 34)
        dOn = np.tile(np.eye(nrow, dtype=dt), (1, H))
        el, er, V, dO = _dev(gpu, el, er, V, dOn)
        want = plain(A, At, gpu, el, er, V, dO, H, 0.2)["dV"].cpu().numpy()
        for drop in (D.PIN_DROP, D.DROP):
            rs = D.rs_of(drop, dt)
            k = D.mask_csr(rp, ci, H, drop, D.SEED)
            got = _gat(A, At, gpu, el, er, V, dO, H, 0.2, drop, D.SEED)["dV"].cpu().numpy()
            for h in range(H):
                sv = slice(h * nrow, (h + 1) * nrow)
                Kt = D.dense_mask(rp, ci, ncol, k[:, h]).T
                exp = np.where(Kt, (want[:, sv] * rs).astype(dt), dt.type(0))
                assert np.array_equal(got[:, sv], exp) and not np.signbit(got[:, sv][~Kt]).any(), (dtype, H, drop, h)
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_sides_form_the_same_ds(crp, gpu, dtype):
    """one entry per column, slope = 1 (g = 1, dZ = dS), one head: d_er[c] of the column side is ds_out of the row side at the
    column's one entry, bit for bit -- s, p, dP', dS and k have the same bits on both sides"""
    rp, ci, ncol = D.one_per_column_matrix()
    nrow = rp.size - 1
    A, At = _handles(rp, ci, nrow, ncol)
    for dv in (5, G.widths(dtype)[3], G.widths(dtype)[5]):
        el, er, V, dO = _dev(gpu, *G.operands(dtype, 1, dv, 2.0, 35, nrow=nrow, ncol=ncol))
        for drop in (D.PIN_DROP, D.DROP):
            got = _gat(A, At, gpu, el, er, V, dO, 1, 1.0, drop, D.SEED)
            ds, d_er = got["ds"].cpu().numpy()[:, 0], got["d_er"].cpu().numpy()[:, 0]
            assert np.array_equal(d_er[ci], ds) and np.abs(ds).max() > 0, (dtype, dv, drop)
            k = D.mask_csr(rp, ci, 1, drop, D.SEED)[:, 0]
            assert (ds[~k] != 0).any(), "a dropped edge still has dS = -p D"
    A.free()
    At.free()


# ---- the bound --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_inside_the_bound(crp, gpu, dtype):
    """every output of every (H, dv) of gat_ref.bound_cases under (DROP, SEED) against the np.longdouble reference, at two scales
    of the scores; the steep rows with bias = 1; the second V block; two sources (forward and row side)"""
    from crp_spmm_amd import hip
    rp, ci = G.matrix()
    A, At = _handles(rp, ci, G.NROW, G.NCOL)
    for dt_, H, dv, spread in D.gat_bound_cases():
        if dt_ != dtype:
            continue
        _, _, el, er, V, dO, ref = D.gat_case(dtype, H, dv, spread)
        el, er, V, dO = _dev(gpu, el, er, V, dO)
        _ratios(_gat(A, At, gpu, el, er, V, dO, H, G.SLOPE, D.DROP, D.SEED), ref, (dtype, "H = %d, dv = %d, spread %g" % (H, dv, spread)))
    A.free()
    At.free()
    rp, ci, val, el, er, V, dO, ref = D.gat_steep_case(dtype)
    A, At = _handles(rp, ci, rp.size - 1, 80, val)
    el, er, V, dO = _dev(gpu, el, er, V, dO)
    got = _gat(A, At, gpu, el, er, V, dO, el.shape[1], G.SLOPE, D.DROP, D.SEED, bias=True)
    _ratios(got, ref, (dtype, "steep rows with bias"))
    masked = np.flatnonzero(~np.isfinite(val))
    assert masked.size and bool((got["p"][masked] == 0).all()) and bool((got["ds"][masked] == 0).all())
    A.free()
    At.free()
    rp, ci, el, er, V, ref = D.gat_second_block_case(dtype)
    A = hip.CsrDev(rp.size - 1, G.NCOL, rp, ci, np.ones(ci.size))
    el, er, V = _dev(gpu, el, er, V)
    _ratios(_gat(A, None, gpu, el, er, V, None, 1, G.SLOPE, D.DROP, D.SEED, backward=False), ref, (dtype, "second V block, dv = %d" % V.shape[1]))
    A.free()
    # two sources: the mask is drawn on the codes as stored
    rp, ci = G.matrix()
    H, dv = 3, G.widths(dtype)[3]
    eln, ern, Vn, dOn = G.operands(dtype, H, dv, 2.0, 36)
    codes = G.two_source_codes(ci)
    ref = D.gat_reference(rp, ci, eln, ern, Vn, G.SLOPE, D.PIN_DROP, D.SEED, None, dOn, codes=codes)
    A2 = hip.CsrDev(G.NROW, G.K0, rp, codes, np.ones(ci.size))
    el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
    got = _gat(A2, None, gpu, el, er[:G.K0], V[:G.K0], dO, H, G.SLOPE, D.PIN_DROP, D.SEED, er1=er[G.K0:], V1=V[G.K0:])
    _ratios(got, ref, (dtype, "two sources, rate %g" % D.PIN_DROP))
    A2.free()


# ---- invariance -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_invariance(crp, gpu, dtype):
    """repeated calls; another seed; with and without the optional outputs; offset pointers and odd leading dimensions (the element
    path against the 16-byte path); dV is V; a row-subset pair against the full handle -- all bit for bit"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.matrix()
    nrow, ncol, nnz = G.NROW, G.NCOL, ci.size
    rows = R.rows_of(rp)
    val = np.random.default_rng(3).standard_normal(nnz)
    A, At = _handles(rp, ci, nrow, ncol, val)
    H = 3
    w = G.W[dtype]
    drop, seed = D.PIN_DROP, D.SEED
    kw = dict(slope=0.2, bias=True, heads=H, dropout=drop, seed=seed)
    for dv in (8 * w, 32 * w + w):
        eln, ern, Vn, dOn = G.operands(dtype, H, dv, 2.0, 31)
        el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
        want = _gat(A, At, gpu, el, er, V, dO, H, 0.2, drop, seed, bias=True)
        _same(_gat(A, At, gpu, el, er, V, dO, H, 0.2, drop, seed, bias=True), want, (dtype, dv, "a repeated call"))
        other = _gat(A, At, gpu, el, er, V, dO, H, 0.2, drop, seed + 1, bias=True)
        assert not torch.equal(other["O"], want["O"]) and not torch.equal(other["dV"], want["dV"]), "another seed, another mask"
        _same(other, want, (dtype, dv, "another seed: lse and p"), keys=("lse", "p"))
        # without the optional outputs
        O = A.gat_attention(el, er, V, **kw)
        d_el, delta = A.gat_attention_bwd_row(el, er, V, want["O"], dO, want["lse"], **kw)
        torch.cuda.synchronize()
        _same(dict(O=O, d_el=d_el, delta=delta), want, (dtype, dv, "without the optional outputs"))
        # offset pointers and odd leading dimensions
        for ld_extra, off in ((1, 0), (0, 1), (3, 1)):
            sel, ser, sV, sdO = (_strided(gpu, t, t.shape[1] + ld_extra, off) for t in (eln, ern, Vn, dOn))
            O = _strided(gpu, np.zeros((nrow, H * dv), dtype), H * dv + ld_extra, off)
            dV = _strided(gpu, np.zeros((ncol, H * dv), dtype), H * dv + ld_extra, off)
            d_el = _strided(gpu, np.zeros((nrow, H), dtype), H + ld_extra, off)
            d_er = _strided(gpu, np.zeros((ncol, H), dtype), H + ld_extra, off)
            lse, p, ds, delta = _nan(gpu, V, nrow, H), _nan(gpu, V, nnz, H), _nan(gpu, V, nnz, H), _nan(gpu, V, nrow, H)
            A.gat_attention(sel, ser, sV, out=O, lse=lse, p_out=p, **kw)
            A.gat_attention_bwd_row(sel, ser, sV, O, sdO, lse, d_el=d_el, delta=delta, ds_out=ds, **kw)
            At.gat_attention_bwd_col(ser, sV, sel, sdO, lse, delta, d_er=d_er, dV=dV, **kw)
            torch.cuda.synchronize()
            got = dict(O=O.contiguous(), lse=lse, p=p, delta=delta, ds=ds, d_el=d_el.contiguous(), d_er=d_er.contiguous(), dV=dV.contiguous())
            _same(got, want, (dtype, dv, "ld + %d, offset %d" % (ld_extra, off)))
        # dV is V on the column side
        Vc = V.clone()
        d_er, dV = At.gat_attention_bwd_col(er, Vc, el, dO, want["lse"], want["delta"], dV=Vc, **kw)
        torch.cuda.synchronize()
        assert dV is Vc
        _same(dict(d_er=d_er, dV=dV), want, (dtype, dv, "dV is V"))
        # a row-subset pair with row maps, writing one set of outputs through its positions: the key holds the mapped row
        O, d_el = _nan(gpu, V, nrow, H * dv), _nan(gpu, V, nrow, H)
        lse, delta, p, ds = _nan(gpu, V, nrow, H), _nan(gpu, V, nrow, H), _nan(gpu, V, nnz, H), _nan(gpu, V, nnz, H)
        pick = (np.arange(nrow) % 4) % 3 == 0
        for sel in (pick, ~pick):
            r = np.flatnonzero(sel)
            keep = sel[rows]
            h = hip.CsrDev(r.size, ncol, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], val[keep])
            h.set_rowmap(r, nrow)
            pos = torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)
            h.gat_attention(el, er, V, out=O, lse=lse, p_out=p, out_pos=pos, **kw)
            h.gat_attention_bwd_row(el, er, V, O, dO, lse, d_el=d_el, delta=delta, ds_out=ds, out_pos=pos, **kw)
            torch.cuda.synchronize()
            h.free()
        _same(dict(O=O, lse=lse, p=p, delta=delta, ds=ds, d_el=d_el), want, (dtype, dv, "row subsets"))
        # NOT claimed: head h of the H-head call against the one-head call on head h's views -- the key holds h
        k = D.mask_csr(rp, ci, H, drop, seed)
        assert (k[:, 1] != k[:, 0]).any()
        one = A.gat_attention(el[:, 1:2].contiguous(), er[:, 1:2].contiguous(), V[:, dv:2 * dv].contiguous(), slope=0.2, bias=True,
                              dropout=drop, seed=seed)
        torch.cuda.synchronize()
        assert not torch.equal(one, want["O"][:, dv:2 * dv])
    A.free()
    At.free()


# ---- special cases ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_special_cases_and_sentinels(crp, gpu, dtype):
    """the wholly dropped row: O = +0 with a finite lse, delta = 0 and a finite d_el; empty, one-entry and all-masked rows; sentinels
    around everything not named stay untouched; NaN in rows no entry names changes nothing"""
    import torch
    dt = np.dtype(dtype)
    rp, ci = G.matrix()
    nrow, ncol, nnz = G.NROW, G.NCOL, ci.size
    lens = np.diff(rp)
    H, dv = 3, 5
    drop, seed = D.DROP, D.SEED
    k = D.mask_csr(rp, ci, H, drop, seed)
    val = np.random.default_rng(12).standard_normal(nnz)
    empty, one = np.flatnonzero(lens == 0), np.flatnonzero(lens == 1)
    dead_row = 3                                                      # a row of 8 entries, all masked
    val[rp[dead_row]:rp[dead_row + 1]] = -np.inf
    gone, gh = 8, 1                                                   # the row of the fixture that is wholly dropped in head 1
    assert lens[gone] >= 2 and not k[rp[gone]:rp[gone + 1], gh].any() and k[rp[gone]:rp[gone + 1], 0].any()
    eln, ern, Vn, dOn = G.operands(dtype, H, dv, 1.5, 61)
    A, At = _handles(rp, ci, nrow, ncol, val)
    el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
    got = _gat(A, At, gpu, el, er, V, dO, H, 0.2, drop, seed, bias=True)
    g = {n: v.cpu().numpy() for n, v in got.items()}
    sv = slice(gh * dv, (gh + 1) * dv)
    assert (g["O"][gone, sv] == 0).all() and not np.signbit(g["O"][gone, sv]).any() and np.isfinite(g["lse"][gone, gh])
    assert g["delta"][gone, gh] == 0 and g["d_el"][gone, gh] == 0 and (g["ds"][rp[gone]:rp[gone + 1], gh] == 0).all()
    assert (g["p"][rp[gone]:rp[gone + 1], gh] > 0).all() and np.abs(g["O"][gone, :dv]).max() > 0
    assert (g["lse"][empty] == -np.inf).all() and (g["O"][empty] == 0).all() and not np.signbit(g["O"][empty]).any()
    assert (g["d_el"][empty] == 0).all() and np.array_equal(g["delta"][empty], np.zeros((empty.size, H)))
    rs = D.rs_of(drop, dt)
    for r in one:
        kept = np.repeat(k[rp[r]], dv)
        assert np.array_equal(g["O"][r], np.where(kept, (Vn[ci[rp[r]]] * rs).astype(dt), 0)), "a one-entry row: O = k ? fl(V[c] rs) : +0"
        assert (g["p"][rp[r]] == 1).all()
    assert (g["lse"][dead_row] == -np.inf).all() and (g["O"][dead_row] == 0).all() and (g["p"][rp[dead_row]:rp[dead_row + 1]] == 0).all()
    assert (g["ds"][rp[dead_row]:rp[dead_row + 1]] == 0).all() and (g["d_el"][dead_row] == 0).all()
    assert (g["d_er"][G.EMPTY_COL] == 0).all() and (g["dV"][G.EMPTY_COL] == 0).all()
    assert all(np.isfinite(g[n]).all() for n in KEYS if n != "lse")
    _ratios(got, D.gat_reference(rp, ci, eln, ern, Vn, 0.2, drop, seed, val, dOn), (dtype, "special cases"))
    # NaN where no entry looks: the er and V rows of a column nobody names, el of the empty rows
    eln2, ern2, Vn2 = eln.copy(), ern.copy(), Vn.copy()
    ern2[G.EMPTY_COL], Vn2[G.EMPTY_COL], eln2[empty] = np.nan, np.nan, np.nan
    el2, er2, V2 = _dev(gpu, eln2, ern2, Vn2)
    _same(_gat(A, At, gpu, el2, er2, V2, dO, H, 0.2, drop, seed, bias=True), got, (dtype, "NaN in rows no entry names"))
    # sentinels: pad columns of O / dV / d_el / d_er, the tails of lse / p_out / delta / ds_out
    pad = 3
    kw = dict(slope=0.2, bias=True, heads=H, dropout=drop, seed=seed)
    mk = lambda r, c: torch.full((r, c), SENT, dtype=V.dtype, device=gpu)
    O, dV, d_el, d_er = mk(nrow + 1, H * dv + pad), mk(ncol + 1, H * dv + pad), mk(nrow + 1, H + pad), mk(ncol + 1, H + pad)
    lse, delta, p, ds = mk(nrow + 1, H), mk(nrow + 1, H), mk(nnz + 1, H), mk(nnz + 1, H)
    A.gat_attention(el, er, V, out=O[:nrow, :H * dv], lse=lse, p_out=p, **kw)
    A.gat_attention_bwd_row(el, er, V, got["O"], dO, got["lse"], d_el=d_el[:nrow, :H], delta=delta, ds_out=ds, **kw)
    At.gat_attention_bwd_col(er, V, el, dO, got["lse"], got["delta"], d_er=d_er[:ncol, :H], dV=dV[:ncol, :H * dv], **kw)
    torch.cuda.synchronize()
    for t, r, c, n in ((O, nrow, H * dv, "O"), (dV, ncol, H * dv, "dV"), (d_el, nrow, H, "d_el"), (d_er, ncol, H, "d_er"), (lse, nrow, H, "lse"),
                       (delta, nrow, H, "delta"), (p, nnz, H, "p"), (ds, nnz, H, "ds")):
        assert torch.equal(t[:r, :c], got[n]), n
        assert bool((t[r:] == SENT).all()) and bool((t[:, c:] == SENT).all()), (n, "a sentinel was overwritten")
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_bad_rate_returns_minus_one_with_nothing_written(crp, gpu, dtype):
    import torch
    lib = crp.load()
    tdt = _tdt(dtype)
    sfx = "f64" if dtype == "float64" else "f32"
    rp, ci = G.matrix()
    nrow, ncol, nnz = 12, G.NCOL, int(rp[12])
    rp, ci = rp[:13], ci[:nnz]
    A, At = _handles(rp, ci, nrow, ncol)
    ffw, frow, fcol = (getattr(lib, "crp_gat_attention_drop_%scsr_%s" % (n, sfx)) for n in ("", "bwd_row_", "bwd_col_"))
    P = lambda t: t.data_ptr()
    H, dv = 2, 8
    wv = H * dv
    el, er, V, O = (torch.ones(s, dtype=tdt, device=gpu) for s in ((nrow, H), (ncol, H), (ncol, wv), (nrow, wv)))
    lse_in = torch.zeros((nrow, H), dtype=tdt, device=gpu)
    for drop, want in ((float("nan"), -1), (-0.25, -1), (1.0, -1), (1.5, -1), (float("inf"), -1), (0.5, 0), (0.0, 0)):
        outs = [torch.full(s, SENT, dtype=tdt, device=gpu) for s in ((nrow, wv), (nrow, H), (nnz, H), (nrow, H), (nrow, H), (nnz, H), (ncol, H),
                                                                      (ncol, wv))]
        Oo, lse, p, d_el, delta, ds, d_er, dV = outs
        mask = torch.full((nnz, H), 9, dtype=torch.uint8, device=gpu)
        rcs = (ffw(A.handle, H, dv, 0.2, 0, P(el), H, P(er), H, None, 0, P(V), wv, None, 0, P(Oo), wv, P(lse), P(p), None, drop, 3, None),
               frow(A.handle, H, dv, 0.2, 0, P(el), H, P(er), H, None, 0, P(V), wv, None, 0, P(O), wv, P(O), wv, P(lse_in), P(d_el), H, P(delta),
                    P(ds), None, drop, 3, None),
               fcol(At.handle, H, dv, 0.2, 0, P(er), H, P(V), wv, P(el), H, P(O), wv, P(lse_in), P(lse_in), P(d_er), H, P(dV), wv, drop, 3, None),
               lib.crp_dropout_mask_csr(A.handle, H, drop, 3, P(mask), None, None))
        torch.cuda.synchronize()
        assert rcs == (want,) * 4, (drop, rcs)
        if want:
            assert all(bool((t == SENT).all()) for t in outs) and bool((mask == 9).all()), (drop, "something was written")
        else:
            assert not any(bool((t == SENT).any()) for t in outs) and not bool((mask == 9).any())
    A.free()
    At.free()


# ---- hip.gat_attention ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_gat_attention_function_against_autograd(crp, gpu, dtype):
    """the gradients of el, er and V through hip.gat_attention(dropout = 0.5, a fixed seed) against torch autograd on an index-based
    fp64 formulation whose edge probabilities are multiplied by numpy's mask times rs, within the sum of the two computations'
    bounds (in the operands' dtype and in fp64); and seed = None under torch.manual_seed reproduces itself"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.matrix()
    nrow, ncol, nnz = G.NROW, G.NCOL, ci.size
    H, dv, slope = 3, 5, 0.2
    drop, seed = 0.5, D.SEED
    A, At = _handles(rp, ci, nrow, ncol)
    eln, ern, Vn, dOn = G.operands(dtype, H, dv, 1.5, 17)
    ref = D.gat_reference(rp, ci, eln, ern, Vn, slope, drop, seed, None, dOn)
    ref64 = D.gat_reference(rp, ci, *(x.astype(np.float64) for x in (eln, ern, Vn)), float(np.dtype(dtype).type(slope)), drop, seed, None,
                            dOn.astype(np.float64))
    el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
    elg, erg, Vg = (t.clone().requires_grad_(True) for t in (el, er, V))
    O = hip.gat_attention(A, At, elg, erg, Vg, slope=slope, heads=H, dropout=drop, seed=seed)
    O.backward(dO)
    torch.cuda.synchronize()
    ri = torch.from_numpy(R.rows_of(rp).astype(np.int64)).to(gpu)
    cj = torch.from_numpy(ci.astype(np.int64)).to(gpu)
    scale = torch.from_numpy(D.mask_csr(rp, ci, H, drop, seed).astype(np.float64) * float(D.rs_of(drop, dtype))).to(gpu)
    e2, r2, V2 = (t.double().clone().requires_grad_(True) for t in (el, er, V))
    s = torch.nn.functional.leaky_relu(e2[ri] + r2[cj], float(np.dtype(dtype).type(slope)))
    m = torch.full((nrow, H), float("-inf"), dtype=torch.float64, device=gpu).scatter_reduce(0, ri[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - m[ri].detach())
    den = torch.zeros((nrow, H), dtype=torch.float64, device=gpu).index_add(0, ri, ex)
    prob = ex / den[ri] * scale
    O2 = torch.zeros((nrow, H, dv), dtype=torch.float64, device=gpu).index_add(0, ri, prob[:, :, None] * V2[cj].view(nnz, H, dv)).view(nrow, H * dv)
    O2.backward(dO.double())
    torch.cuda.synchronize()
    for n, mine, theirs in (("O", O.detach(), O2.detach()), ("d_el", elg.grad, e2.grad), ("d_er", erg.grad, r2.grad), ("dV", Vg.grad, V2.grad)):
        tol = (ref[n][1] + ref64[n][1]).astype(np.float64)
        err = np.abs(mine.double().cpu().numpy() - theirs.cpu().numpy())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0))
        print("%s %s: worst |hip - autograd| / (sum of the bounds) %.3g" % (dtype, n, ratio.max()))
        assert ratio.max() <= 1, (dtype, n, float(ratio.max()))
    # seed = None: 64 bits from torch's default host generator, so torch.manual_seed reproduces the run; dropout = 0 draws nothing
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        runs.append(hip.gat_attention(A, At, el, er, V, slope=slope, heads=H, dropout=drop))
    again = hip.gat_attention(A, At, el, er, V, slope=slope, heads=H, dropout=drop)
    state = torch.get_rng_state()
    plain = hip.gat_attention(A, At, el, er, V, slope=slope, heads=H)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]) and not torch.equal(again, runs[0]) and torch.equal(torch.get_rng_state(), state)
    assert torch.equal(plain, A.gat_attention(el, er, V, slope=slope, heads=H))
    A.free()
    At.free()
