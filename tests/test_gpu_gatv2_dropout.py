"""GPU: attention dropout in the fused GATv2 attention and its two-handle backward (crp_gatv2_attention_drop_csr_*, _bwd_row_,
_bwd_col_, the CsrDev keywords and hip.gatv2_attention(dropout=, seed=)).

dropout = 0 against the existing calls, bit for bit.  Exact pins against the kernels that exist (torch.equal, nothing compared with
the code under test): with XS = I (which also feeds the score, identically in both runs) every column of O holds one entry's term,
so O_drop == where(k, fl(O_plain rs), +0); lse and p_out are the plain call's; with a = 0 (accZ = 0) and dO = I on the column side
dXS_drop == where(k, fl(dXS_plain rs), +0).  Then everything inside the bound of DESIGN.md 5q against
tests/dropout_ref.gatv2_reference, the invariances, the special cases and hip.gatv2_attention against torch autograd.  The mask
itself is pinned in tests/test_gpu_gat_dropout.py.

Head h of an H-head call is NOT the one-head call on head h's views under dropout: the key of the draw holds h.  That invariance
of 5n is not claimed here."""
import numpy as np
import pytest

import attention_ref as R
import dropout_ref as D
import gat_ref as G
import gatv2_ref as G2
from test_gpu_attention import SENT, _strided, _tdt
from test_gpu_gatv2 import _dev, _handles, _nan, _same

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
KEYS = G2.FWD_KEYS + G2.BWD_KEYS


def _g2(A, At, gpu, XT, XS, a, dO, H, slope, drop, seed, bias=False, XS1=None, backward=True):
    """one forward, row side, col_sum and (At given) column side under dropout -> dict of device tensors"""
    import torch
    from crp_spmm_amd import hip
    nrow, nnz = XT.shape[0], A.nnz
    kw = dict(slope=slope, bias=bias, heads=H, dropout=drop, seed=seed)
    lse, p = _nan(gpu, XT, nrow, H), _nan(gpu, XT, nnz, H)
    O = A.gatv2_attention(XT, XS, a, XS1=XS1, lse=lse, p_out=p, **kw)
    out = dict(O=O, lse=lse, p=p)
    if backward:
        ds = _nan(gpu, XT, nnz, H)
        dXT, da_part, delta = A.gatv2_attention_bwd_row(XT, XS, a, O, dO, lse, XS1=XS1, ds_out=ds, **kw)
        out.update(delta=delta, ds=ds, dXT=dXT, da_part=da_part, da=hip.col_sum(da_part))
        if At is not None:
            out.update(dXS=At.gatv2_attention_bwd_col(XS, XT, a, dO, lse, delta, **kw))
    torch.cuda.synchronize()
    return out


def _ratios(got, ref, what):
    r = D.ratios({k: v.cpu().numpy() for k, v in got.items()}, ref)
    print("%s: worst |got - ref| / bound  %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) <= 1, (what, r)
    return r


# ---- dropout = 0 and the exact pins -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_zero_is_the_existing_call(crp, gpu, dtype):
    from test_gpu_gatv2 import _g2 as plain
    rp, ci = G2.matrix()
    val = np.random.default_rng(8).standard_normal(ci.size)
    A, At = _handles(rp, ci, G2.NROW, G2.NCOL, val)
    for i, dv in enumerate(G2.widths(dtype)):
        H = (1, 3)[i % 2]
        XT, XS, a, dO = _dev(gpu, *G2.operands(dtype, H, dv, 2.0, 40 + i))
        want = plain(A, At, gpu, XT, XS, a, dO, H, 0.2, bias=True)
        _same(_g2(A, At, gpu, XT, XS, a, dO, H, 0.2, 0.0, D.SEED, bias=True), want, (dtype, H, dv, "dropout = 0"))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_with_identity_sources_and_lse_and_p_out(crp, gpu, dtype):
    """XS = I (dv = the number of columns; it feeds the score too, identically in both runs): O_drop == where(k, fl(O_plain rs), +0)
    bit for bit, on the 40 x 80 matrix and on an 8-column one (the group of 8 lanes); lse and p_out are the existing call's"""
    from test_gpu_gatv2 import _g2 as plain
    dt = np.dtype(dtype)
    for (rp, ci, ncol), H in (((*G.matrix(), G.NCOL), 1), ((*G.matrix(), G.NCOL), 3), (D.narrow_matrix(), 1), (D.narrow_matrix(), 3)):
        nrow = rp.size - 1
        A, _ = _handles(rp, ci, nrow, ncol)
        XT, _, a, _ = G2.operands(dtype, H, ncol, 2.0, 33, nrow=nrow, ncol=ncol)
        XT, XS, a = _dev(gpu, XT, np.tile(np.eye(ncol, dtype=dt), (1, H)), a)
        want = plain(A, None, gpu, XT, XS, a, None, H, 0.2, backward=False)
        On = want["O"].cpu().numpy()
        for drop in (D.PIN_DROP, D.DROP, 0.9):
            rs = D.rs_of(drop, dt)
            k = D.mask_csr(rp, ci, H, drop, D.SEED)
            got = _g2(A, None, gpu, XT, XS, a, None, H, 0.2, drop, D.SEED, backward=False)
            _same(got, want, (dtype, H, ncol, drop, "lse and p_out"), keys=("lse", "p"))
            for h in range(H):
                sv = slice(h * ncol, (h + 1) * ncol)
                K = D.dense_mask(rp, ci, ncol, k[:, h])
                exp = np.where(K, (On[:, sv] * rs).astype(dt), dt.type(0))
                mine = got["O"][:, sv].cpu().numpy()
                assert np.array_equal(mine, exp) and not np.signbit(mine[~K]).any(), (dtype, H, ncol, drop, h)
        A.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_side_with_identity_gradient_and_a_zero(crp, gpu, dtype):
    """a = 0 (every score 0, accZ = 0) and dO rows as unit vectors (dv = the number of rows): dXS_drop == where(k, fl(dXS_plain rs),
    +0) bit for bit"""
    from test_gpu_gatv2 import _g2 as plain
    dt = np.dtype(dtype)
    rp, ci = G.matrix()
    nrow, ncol = G.NROW, G.NCOL
    A, At = _handles(rp, ci, nrow, ncol)
    for H in (1, 3):
        XT, XS, a, _ = G2.operands(dtype, H, nrow, 2.0, 34)
        dOn = np.tile(np.eye(nrow, dtype=dt), (1, H))
        XT, XS, a, dO = _dev(gpu, XT, XS, np.zeros_like(a), dOn)
        want = plain(A, At, gpu, XT, XS, a, dO, H, 0.2)["dXS"].cpu().numpy()
        for drop in (D.PIN_DROP, D.DROP):
            rs = D.rs_of(drop, dt)
            k = D.mask_csr(rp, ci, H, drop, D.SEED)
            got = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, drop, D.SEED)["dXS"].cpu().numpy()
            for h in range(H):
                sv = slice(h * nrow, (h + 1) * nrow)
                Kt = D.dense_mask(rp, ci, ncol, k[:, h]).T
                exp = np.where(Kt, (want[:, sv] * rs).astype(dt), dt.type(0))
                assert np.array_equal(got[:, sv], exp), (dtype, H, drop, h)
    A.free()
    At.free()


# ---- the bound --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_inside_the_bound(crp, gpu, dtype):
    """every output of every (H, dv) of gatv2_ref.bound_cases below the cap under (DROP, SEED) against the np.longdouble reference,
    at two scales of the scores; the steep rows with bias = 1; two sources (forward and row side)"""
    from crp_spmm_amd import hip
    rp, ci = G2.matrix()
    A, At = _handles(rp, ci, G2.NROW, G2.NCOL)
    for dt_, H, dv, spread, short in D.gatv2_bound_cases():
        if dt_ != dtype:
            continue
        _, _, XT, XS, a, dO, ref = D.gatv2_case(dtype, H, dv, spread, short)
        XT, XS, a, dO = _dev(gpu, XT, XS, a, dO)
        _ratios(_g2(A, At, gpu, XT, XS, a, dO, H, G2.SLOPE, D.DROP, D.SEED), ref, (dtype, "H = %d, dv = %d, spread %g" % (H, dv, spread)))
    A.free()
    At.free()
    rp, ci, val, XT, XS, a, dO, ref = D.gatv2_steep_case(dtype)
    A, At = _handles(rp, ci, rp.size - 1, 80, val)
    XT, XS, a, dO = _dev(gpu, XT, XS, a, dO)
    got = _g2(A, At, gpu, XT, XS, a, dO, a.shape[0], G2.SLOPE, D.DROP, D.SEED, bias=True)
    _ratios(got, ref, (dtype, "steep rows with bias"))
    masked = np.flatnonzero(~np.isfinite(val))
    assert masked.size and bool((got["p"][masked] == 0).all()) and bool((got["ds"][masked] == 0).all())
    A.free()
    At.free()
    rp, ci = G2.matrix()
    H, dv = 3, G2.widths(dtype)[3]
    XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 2.0, 36)
    codes = G2.two_source_codes(ci)
    ref = D.gatv2_reference(rp, ci, XTn, XSn, an, G2.SLOPE, D.PIN_DROP, D.SEED, None, dOn, codes=codes)
    A2 = hip.CsrDev(G2.NROW, G2.K0, rp, codes, np.ones(ci.size))
    XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
    got = _g2(A2, None, gpu, XT, XS[:G2.K0], a, dO, H, G2.SLOPE, D.PIN_DROP, D.SEED, XS1=XS[G2.K0:])
    _ratios(got, ref, (dtype, "two sources, rate %g" % D.PIN_DROP))
    A2.free()


# ---- invariance -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_invariance(crp, gpu, dtype):
    """repeated calls; another seed; with and without the optional outputs; offset pointers and odd leading dimensions (the element
    path against the 16-byte path); dXS is XS; a row-subset pair against the full handle -- all bit for bit"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
    rows = R.rows_of(rp)
    val = np.random.default_rng(3).standard_normal(nnz)
    A, At = _handles(rp, ci, nrow, ncol, val)
    H = 3
    w = G2.W[dtype]
    drop, seed = D.PIN_DROP, D.SEED
    kw = dict(slope=0.2, bias=True, heads=H, dropout=drop, seed=seed)
    for dv in (8 * w, 32 * w + w):
        XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 2.0, 31)
        XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
        want = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, drop, seed, bias=True)
        _same(_g2(A, At, gpu, XT, XS, a, dO, H, 0.2, drop, seed, bias=True), want, (dtype, dv, "a repeated call"))
        other = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, drop, seed + 1, bias=True)
        assert not torch.equal(other["O"], want["O"]) and not torch.equal(other["dXS"], want["dXS"]), "another seed, another mask"
        _same(other, want, (dtype, dv, "another seed: lse and p"), keys=("lse", "p"))
        # without the optional outputs
        O = A.gatv2_attention(XT, XS, a, **kw)
        dXT, da_part, delta = A.gatv2_attention_bwd_row(XT, XS, a, want["O"], dO, want["lse"], **kw)
        torch.cuda.synchronize()
        _same(dict(O=O, dXT=dXT, da_part=da_part, delta=delta), want, (dtype, dv, "without the optional outputs"))
        # offset pointers and odd leading dimensions (a stays contiguous: the element path is taken through the others)
        for ld_extra, off in ((1, 0), (0, 1), (3, 1)):
            sXT, sXS, sdO = (_strided(gpu, t, t.shape[1] + ld_extra, off) for t in (XTn, XSn, dOn))
            z = lambda r: _strided(gpu, np.zeros((r, H * dv), dtype), H * dv + ld_extra, off)
            O, dXT, da_part, dXS = z(nrow), z(nrow), z(nrow), z(ncol)
            lse, p, ds, delta = _nan(gpu, XT, nrow, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nrow, H)
            A.gatv2_attention(sXT, sXS, a, out=O, lse=lse, p_out=p, **kw)
            A.gatv2_attention_bwd_row(sXT, sXS, a, O, sdO, lse, dXT=dXT, da_part=da_part, delta=delta, ds_out=ds, **kw)
            At.gatv2_attention_bwd_col(sXS, sXT, a, sdO, lse, delta, dXS=dXS, **kw)
            torch.cuda.synchronize()
            got = dict(O=O.contiguous(), lse=lse, p=p, delta=delta, ds=ds, dXT=dXT.contiguous(), da_part=da_part.contiguous(),
                       dXS=dXS.contiguous())
            _same(got, want, (dtype, dv, "ld + %d, offset %d" % (ld_extra, off)))
        # dXS is XS on the column side
        Xc = XS.clone()
        dXS = At.gatv2_attention_bwd_col(Xc, XT, a, dO, want["lse"], want["delta"], dXS=Xc, **kw)
        torch.cuda.synchronize()
        assert dXS is Xc
        _same(dict(dXS=dXS), want, (dtype, dv, "dXS is XS"))
        # a row-subset pair with row maps, writing one set of outputs through its positions: the key holds the mapped row
        O, dXT, da_part = _nan(gpu, XT, nrow, H * dv), _nan(gpu, XT, nrow, H * dv), _nan(gpu, XT, nrow, H * dv)
        lse, delta, p, ds = _nan(gpu, XT, nrow, H), _nan(gpu, XT, nrow, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nnz, H)
        pick = (np.arange(nrow) % 4) % 3 == 0
        for sel in (pick, ~pick):
            r = np.flatnonzero(sel)
            keep = sel[rows]
            h = hip.CsrDev(r.size, ncol, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], val[keep])
            h.set_rowmap(r, nrow)
            pos = torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)
            h.gatv2_attention(XT, XS, a, out=O, lse=lse, p_out=p, out_pos=pos, **kw)
            h.gatv2_attention_bwd_row(XT, XS, a, O, dO, lse, dXT=dXT, da_part=da_part, delta=delta, ds_out=ds, out_pos=pos, **kw)
            torch.cuda.synchronize()
            h.free()
        _same(dict(O=O, lse=lse, p=p, delta=delta, ds=ds, dXT=dXT, da_part=da_part), want, (dtype, dv, "row subsets"))
    A.free()
    At.free()


# ---- special cases ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_special_cases_and_sentinels(crp, gpu, dtype):
    """the wholly dropped row: O = +0 with a finite lse, delta = 0 and finite dXT / da_part; empty, one-entry and all-masked rows;
    sentinels around everything not named stay untouched; NaN in rows no entry names changes nothing"""
    import torch
    dt = np.dtype(dtype)
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
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
    XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 1.5, 61)
    A, At = _handles(rp, ci, nrow, ncol, val)
    XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
    got = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, drop, seed, bias=True)
    g = {n: v.cpu().numpy() for n, v in got.items()}
    sv = slice(gh * dv, (gh + 1) * dv)
    assert (g["O"][gone, sv] == 0).all() and not np.signbit(g["O"][gone, sv]).any() and np.isfinite(g["lse"][gone, gh])
    assert g["delta"][gone, gh] == 0 and (g["dXT"][gone, sv] == 0).all() and (g["ds"][rp[gone]:rp[gone + 1], gh] == 0).all()
    assert (g["p"][rp[gone]:rp[gone + 1], gh] > 0).all() and np.abs(g["O"][gone, :dv]).max() > 0
    assert (g["lse"][empty] == -np.inf).all() and (g["O"][empty] == 0).all() and not np.signbit(g["O"][empty]).any()
    assert (g["dXT"][empty] == 0).all() and (g["da_part"][empty] == 0).all() and np.array_equal(g["delta"][empty], np.zeros((empty.size, H)))
    rs = D.rs_of(drop, dt)
    for r in one:
        kept = np.repeat(k[rp[r]], dv)
        assert np.array_equal(g["O"][r], np.where(kept, (XSn[ci[rp[r]]] * rs).astype(dt), 0)), "a one-entry row: O = k ? fl(XS[c] rs) : +0"
        assert (g["p"][rp[r]] == 1).all()
    assert (g["lse"][dead_row] == -np.inf).all() and (g["O"][dead_row] == 0).all() and (g["p"][rp[dead_row]:rp[dead_row + 1]] == 0).all()
    assert (g["ds"][rp[dead_row]:rp[dead_row + 1]] == 0).all() and (g["dXT"][dead_row] == 0).all()
    assert (g["dXS"][G2.EMPTY_COL] == 0).all()
    assert all(np.isfinite(g[n]).all() for n in KEYS if n != "lse")
    _ratios(got, D.gatv2_reference(rp, ci, XTn, XSn, an, 0.2, drop, seed, val, dOn), (dtype, "special cases"))
    # NaN where no entry looks: the XS row of a column nobody names, XT of the empty rows
    XTn2, XSn2 = XTn.copy(), XSn.copy()
    XSn2[G2.EMPTY_COL], XTn2[empty] = np.nan, np.nan
    XT2, XS2 = _dev(gpu, XTn2, XSn2)
    again = _g2(A, At, gpu, XT2, XS2, a, dO, H, 0.2, drop, seed, bias=True)
    _same(again, got, (dtype, "NaN in rows no entry names"))
    # sentinels: pad columns of O / dXT / da_part / dXS, the tails of lse / p_out / delta / ds_out
    pad = 3
    kw = dict(slope=0.2, bias=True, heads=H, dropout=drop, seed=seed)
    mk = lambda r, c: torch.full((r, c), SENT, dtype=XT.dtype, device=gpu)
    O, dXT, dap, dXS = mk(nrow + 1, H * dv + pad), mk(nrow + 1, H * dv + pad), mk(nrow + 1, H * dv + pad), mk(ncol + 1, H * dv + pad)
    lse, delta, p, ds = mk(nrow + 1, H), mk(nrow + 1, H), mk(nnz + 1, H), mk(nnz + 1, H)
    A.gatv2_attention(XT, XS, a, out=O[:nrow, :H * dv], lse=lse, p_out=p, **kw)
    A.gatv2_attention_bwd_row(XT, XS, a, got["O"], dO, got["lse"], dXT=dXT[:nrow, :H * dv], da_part=dap[:nrow, :H * dv], delta=delta,
                              ds_out=ds, **kw)
    At.gatv2_attention_bwd_col(XS, XT, a, dO, got["lse"], got["delta"], dXS=dXS[:ncol, :H * dv], **kw)
    torch.cuda.synchronize()
    for t, r, c, n in ((O, nrow, H * dv, "O"), (dXT, nrow, H * dv, "dXT"), (dap, nrow, H * dv, "da_part"), (dXS, ncol, H * dv, "dXS"),
                       (lse, nrow, H, "lse"), (delta, nrow, H, "delta"), (p, nnz, H, "p"), (ds, nnz, H, "ds")):
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
    rp, ci = G2.matrix()
    nrow, ncol, nnz = 12, G2.NCOL, int(rp[12])
    rp, ci = rp[:13], ci[:nnz]
    A, At = _handles(rp, ci, nrow, ncol)
    ffw, frow, fcol = (getattr(lib, "crp_gatv2_attention_drop_%scsr_%s" % (n, sfx)) for n in ("", "bwd_row_", "bwd_col_"))
    P = lambda t: t.data_ptr()
    H, dv = 2, 8
    wv = H * dv
    XT, XS, O = (torch.ones(s, dtype=tdt, device=gpu) for s in ((nrow, wv), (ncol, wv), (nrow, wv)))
    a = torch.ones(wv, dtype=tdt, device=gpu)
    lse_in = torch.zeros((nrow, H), dtype=tdt, device=gpu)
    for drop, want in ((float("nan"), -1), (-0.25, -1), (1.0, -1), (1.5, -1), (float("inf"), -1), (0.5, 0), (0.0, 0)):
        outs = [torch.full(s, SENT, dtype=tdt, device=gpu) for s in ((nrow, wv), (nrow, H), (nnz, H), (nrow, wv), (nrow, wv), (nrow, H), (nnz, H),
                                                                      (ncol, wv))]
        Oo, lse, p, dXT, dap, delta, ds, dXS = outs
        rcs = (ffw(A.handle, H, dv, 0.2, 0, P(XT), wv, P(XS), wv, None, 0, P(a), P(Oo), wv, P(lse), P(p), None, drop, 3, None),
               frow(A.handle, H, dv, 0.2, 0, P(XT), wv, P(XS), wv, None, 0, P(a), P(O), wv, P(O), wv, P(lse_in), P(dXT), wv, P(dap), wv,
                    P(delta), P(ds), None, drop, 3, None),
               fcol(At.handle, H, dv, 0.2, 0, P(XS), wv, P(XT), wv, P(a), P(O), wv, P(lse_in), P(lse_in), P(dXS), wv, drop, 3, None))
        torch.cuda.synchronize()
        assert rcs == (want,) * 3, (drop, rcs)
        if want:
            assert all(bool((t == SENT).all()) for t in outs), (drop, "something was written")
        else:
            assert not any(bool((t == SENT).any()) for t in outs)
    A.free()
    At.free()


# ---- hip.gatv2_attention ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_gatv2_attention_function_against_autograd(crp, gpu, dtype):
    """the gradients of XT, XS and a through hip.gatv2_attention(dropout = 0.5, a fixed seed) against torch autograd on an
    index-based fp64 formulation whose edge probabilities are multiplied by numpy's mask times rs, within the sum of the two
    computations' bounds (in the operands' dtype and in fp64); and seed = None under torch.manual_seed reproduces itself"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
    H, dv, slope = 3, 5, 0.2
    drop, seed = 0.5, D.SEED
    A, At = _handles(rp, ci, nrow, ncol)
    XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 1.5, 17)
    sl = float(np.dtype(dtype).type(slope))
    ref = D.gatv2_reference(rp, ci, XTn, XSn, an, slope, drop, seed, None, dOn)
    ref64 = D.gatv2_reference(rp, ci, *(x.astype(np.float64) for x in (XTn, XSn, an)), sl, drop, seed, None, dOn.astype(np.float64))
    XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
    XTg, XSg, ag = (t.clone().requires_grad_(True) for t in (XT, XS, a))
    O = hip.gatv2_attention(A, At, XTg, XSg, ag, slope=slope, heads=H, dropout=drop, seed=seed)
    O.backward(dO)
    torch.cuda.synchronize()
    ri = torch.from_numpy(R.rows_of(rp).astype(np.int64)).to(gpu)
    cj = torch.from_numpy(ci.astype(np.int64)).to(gpu)
    scale = torch.from_numpy(D.mask_csr(rp, ci, H, drop, seed).astype(np.float64) * float(D.rs_of(drop, dtype))).to(gpu)
    T2, S2, a2 = (t.double().clone().requires_grad_(True) for t in (XT, XS, a))
    r = torch.nn.functional.leaky_relu(T2[ri] + S2[cj], sl).view(nnz, H, dv)
    s = (r * a2[None, :, :]).sum(dim=2)
    m = torch.full((nrow, H), float("-inf"), dtype=torch.float64, device=gpu).scatter_reduce(0, ri[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - m[ri].detach())
    den = torch.zeros((nrow, H), dtype=torch.float64, device=gpu).index_add(0, ri, ex)
    prob = ex / den[ri] * scale
    O2 = torch.zeros((nrow, H, dv), dtype=torch.float64, device=gpu).index_add(0, ri, prob[:, :, None] * S2[cj].view(nnz, H, dv)).view(nrow, H * dv)
    O2.backward(dO.double())
    torch.cuda.synchronize()
    # dXS of the function is the gradient of XS through both of its uses: the reference's dXS
    for n, mine, theirs in (("O", O.detach(), O2.detach()), ("dXT", XTg.grad, T2.grad), ("dXS", XSg.grad, S2.grad),
                            ("da", ag.grad.reshape(-1), a2.grad.reshape(-1))):
        tol = (ref[n][1] + ref64[n][1]).astype(np.float64)
        err = np.abs(mine.double().cpu().numpy() - theirs.cpu().numpy())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0))
        print("%s %s: worst |hip - autograd| / (sum of the bounds) %.3g" % (dtype, n, ratio.max()))
        assert ratio.max() <= 1, (dtype, n, float(ratio.max()))
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        runs.append(hip.gatv2_attention(A, At, XT, XS, a, slope=slope, heads=H, dropout=drop))
    again = hip.gatv2_attention(A, At, XT, XS, a, slope=slope, heads=H, dropout=drop)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]) and not torch.equal(again, runs[0])
    A.free()
    At.free()
