"""GPU: the fused GAT attention and its two-handle backward (crp_gat_attention_csr_*, crp_gat_attention_bwd_row_csr_*,
crp_gat_attention_bwd_col_csr_*, the CsrDev wrappers and hip.gat_attention).

Bit pins against the kernels that exist (torch.equal, no tolerance, nothing compared with the code under test):
  slope = 1          the fused attention with dk = 2 on Q_h = [el_h, 1], K_h = [1, er_h], scale = 1 forms fl(el + er) as its dot, so
                     O, lse, p_out, delta, ds_out and dV are its outputs, d_el[:, h] = dQ_h[:, 0] and d_er[:, h] = dK_h[:, 1];
  any slope          the single-head attention with Q = 0 and bias = 1 on a handle whose values are lrelu(fl(el + er)), formed by
                     numpy in the dtype (exact in the handle's fp64 store and in its fp32 copy); d_el and d_er are numpy's
                     sequential sums, in the dtype, of that run's ds_out times g;
  bias = 1           the same on exact data (small integers, slope 1/4, integer values), where a + val is exact.
Then everything inside the bound of DESIGN.md 5o against tests/gat_ref.reference, the invariances, the special cases and
hip.gat_attention against torch autograd.  Pattern: gat_ref.matrix(), 40 x 80 with rows of 0, 1, 7, 8, 9, 17 and 70 entries."""
import numpy as np
import pytest

import attention_bwd_ref as B
import attention_ref as R
import gat_ref as G
from test_gpu_attention import SENT, _strided, _tdt

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
KEYS = G.FWD_KEYS + G.BWD_KEYS
SLOPES = (0.2, 0.25, 0.0)


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.array(a, order="C")).to(gpu) for a in arrays]


def _nan(gpu, like, *shape):
    import torch
    return torch.full(shape, float("nan"), dtype=like.dtype, device=gpu)


def _handles(rp, ci, nrow, ncol, val=None):
    from crp_spmm_amd import hip
    val = np.ones(ci.size) if val is None else val
    return hip.CsrDev(nrow, ncol, rp, ci, val), hip.CsrDev.from_transpose(nrow, ncol, rp, ci, val)


def _gat(A, At, gpu, el, er, V, dO, H, slope, bias=False, er1=None, V1=None, backward=True):
    """one forward, row side and (At given) column side -> dict of device tensors, every output asked for"""
    import torch
    nrow, nnz = el.shape[0], A.nnz
    lse, p = _nan(gpu, V, nrow, H), _nan(gpu, V, nnz, H)
    O = A.gat_attention(el, er, V, er1=er1, V1=V1, slope=slope, bias=bias, lse=lse, p_out=p, heads=H)
    out = dict(O=O, lse=lse, p=p)
    if backward:
        ds = _nan(gpu, V, nnz, H)
        d_el, delta = A.gat_attention_bwd_row(el, er, V, O, dO, lse, er1=er1, V1=V1, slope=slope, bias=bias, ds_out=ds, heads=H)
        out.update(delta=delta, ds=ds, d_el=d_el)
        if At is not None:
            d_er, dV = At.gat_attention_bwd_col(er, V, el, dO, lse, delta, slope=slope, bias=bias, heads=H)
            out.update(d_er=d_er, dV=dV)
    torch.cuda.synchronize()
    return out


def _same(got, want, what, keys=KEYS):
    import torch
    for k in keys:
        if k in got and k in want:
            assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
            assert torch.equal(got[k], want[k]), (what, k, "differs")


def _cases(dtype):
    for i, dv in enumerate(G.widths(dtype)):
        for H in (1, 3):
            yield i, H, dv


# ---- bit pins ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_slope_one_equals_the_attention_with_two_columns(crp, gpu, dtype):
    import torch
    rp, ci = G.matrix()
    val = np.random.default_rng(8).standard_normal(ci.size)
    A, At = _handles(rp, ci, G.NROW, G.NCOL, val)
    for i, H, dv in _cases(dtype):
        el, er, V, dO = _dev(gpu, *G.operands(dtype, H, dv, 2.0, 50 + i))
        Q = torch.ones((G.NROW, 2 * H), dtype=V.dtype, device=gpu)
        K = torch.ones((G.NCOL, 2 * H), dtype=V.dtype, device=gpu)
        Q[:, 0::2], K[:, 1::2] = el, er
        for bias in (False, True):
            lse, p, ds = _nan(gpu, V, G.NROW, H), _nan(gpu, V, ci.size, H), _nan(gpu, V, ci.size, H)
            flat = (lambda t: t.view(-1)) if H == 1 else (lambda t: t)
            O = A.attention(Q, K, V, scale=1.0, bias=bias, lse=flat(lse), p_out=flat(p), heads=H)
            dQ, delta = A.attention_bwd_q(Q, K, V, O, dO, flat(lse), scale=1.0, bias=bias, ds_out=flat(ds), heads=H)
            dK, dV = At.attention_bwd_kv(K, V, Q, dO, flat(lse), flat(delta), scale=1.0, bias=bias, heads=H)
            torch.cuda.synchronize()
            want = dict(O=O, lse=lse, p=p, delta=delta.view(G.NROW, H), ds=ds, d_el=dQ[:, 0::2].contiguous(), d_er=dK[:, 1::2].contiguous(), dV=dV)
            got = _gat(A, At, gpu, el, er, V, dO, H, 1.0, bias=bias)
            got["d_el"], got["d_er"] = got["d_el"].contiguous(), got["d_er"].contiguous()
            _same(got, want, (dtype, H, dv, "bias" if bias else "no bias"))
            assert all(bool(got[k].isfinite().all()) for k in KEYS if k != "lse")
    A.free()
    At.free()


def _pin_by_values(gpu, dtype, rp, ci, nrow, ncol, A, At, Av, Atv, el, er, V, dO, H, slope, val=None):
    """the GAT calls on (A, At) against the single-head attention with Q = 0, bias = 1 on (Av, Atv), whose values become the scores
    numpy forms in the dtype, head by head"""
    import torch
    dt = np.dtype(dtype)
    dv = V.shape[1] // H
    eln, ern = el.cpu().numpy(), er.cpu().numpy()
    got = _gat(A, At, gpu, el, er, V, dO, H, slope, bias=val is not None)
    rpt, cit, tmap = B.transpose(rp, ci, ncol)
    Q0 = torch.zeros((nrow, 1), dtype=V.dtype, device=gpu)
    K0 = torch.zeros((ncol, 1), dtype=V.dtype, device=gpu)
    for h in range(H):
        s, g = G.scores_dtype(rp, ci, eln, ern, slope, h, val)
        s64 = s.astype(np.float64)
        assert np.array_equal(s64.astype(dt), s, equal_nan=True), "the values are exact in fp64 and in the fp32 copy"
        Av.update_values(s64)
        Atv.update_values(s64)
        sv = slice(h * dv, (h + 1) * dv)
        Vh, dOh = V[:, sv], dO[:, sv]
        lse, p, ds = _nan(gpu, V, nrow), _nan(gpu, V, ci.size), _nan(gpu, V, ci.size)
        O = Av.attention(Q0, K0, Vh, scale=1.0, bias=True, lse=lse, p_out=p)
        _, delta = Av.attention_bwd_q(Q0, K0, Vh, O, dOh, lse, scale=1.0, bias=True, ds_out=ds)
        _, dV = Atv.attention_bwd_kv(K0, Vh, Q0, dOh, lse, delta, scale=1.0, bias=True)
        torch.cuda.synchronize()
        dsn = ds.cpu().numpy()
        with np.errstate(invalid="ignore"):
            dz = np.where(dsn == 0, 0, dsn * g).astype(dt)
        want = dict(O=O, lse=lse, p=p, delta=delta, ds=ds, dV=dV, d_el=_dev(gpu, G.seq_sum(rp, dz))[0], d_er=_dev(gpu, G.seq_sum(rpt, dz[tmap]))[0])
        mine = dict(O=got["O"][:, sv], lse=got["lse"][:, h], p=got["p"][:, h], delta=got["delta"][:, h], ds=got["ds"][:, h],
                    dV=got["dV"][:, sv], d_el=got["d_el"][:, h], d_er=got["d_er"][:, h])
        _same(mine, want, (dtype, "H = %d, dv = %d, slope %g, head %d" % (H, dv, slope, h)))
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_any_slope_equals_the_attention_on_scores_as_values(crp, gpu, dtype):
    rp, ci = G.matrix()
    A, At = _handles(rp, ci, G.NROW, G.NCOL)
    Av, Atv = _handles(rp, ci, G.NROW, G.NCOL)
    for i, H, dv in _cases(dtype):
        el, er, V, dO = _dev(gpu, *G.operands(dtype, H, dv, 3.0, 70 + i))
        for slope in (SLOPES if i in (1, 3) else (SLOPES[i % 3],)):
            got = _pin_by_values(gpu, dtype, rp, ci, G.NROW, G.NCOL, A, At, Av, Atv, el, er, V, dO, H, slope)
            assert all(bool(got[k].isfinite().all()) for k in KEYS if k != "lse")
    for h in (A, At, Av, Atv):
        h.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_with_a_slope_on_exact_data(crp, gpu, dtype):
    """small integers, slope 1/4 and integer values: z, slope z and a + val are exact, so a contracted slope z + val would give the
    same bits here -- and the values of the reference handle are the exact scores; the contraction itself is caught by the inexact
    data of test_bias_is_added_after_its_own_rounding"""
    rp, ci = G.matrix()
    rng = np.random.default_rng(4)
    val = rng.integers(-4, 5, ci.size).astype(np.float64)
    A, At = _handles(rp, ci, G.NROW, G.NCOL, val)
    Av, Atv = _handles(rp, ci, G.NROW, G.NCOL)
    for i, H, dv in _cases(dtype):
        _, _, V, dO = G.operands(dtype, H, dv, 1.0, 90 + i)
        el = rng.integers(-8, 9, (G.NROW, H)).astype(dtype)
        er = rng.integers(-8, 9, (G.NCOL, H)).astype(dtype)
        el, er, V, dO = _dev(gpu, el, er, V, dO)
        _pin_by_values(gpu, dtype, rp, ci, G.NROW, G.NCOL, A, At, Av, Atv, el, er, V, dO, H, 0.25, val)
    for h in (A, At, Av, Atv):
        h.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_is_added_after_its_own_rounding(crp, gpu, dtype):
    """inexact data with bias = 1: the reference handle carries fl(fl(slope z) + val), which numpy forms in two roundings; a kernel
    that contracted slope z + val into an FMA differs in some entry"""
    rp, ci = G.matrix()
    dt = np.dtype(dtype)
    val = np.random.default_rng(6).standard_normal(ci.size).astype(dt).astype(np.float64)
    el, er, _, _ = G.operands(dtype, 1, 1, 3.0, 5)
    rows = R.rows_of(rp)
    z = (el[rows, 0] + er[ci, 0]).astype(dt)
    sl = dt.type(0.2)
    two = ((sl * z).astype(dt) + val.astype(dt)).astype(dt)
    one = (np.longdouble(sl) * z.astype(np.longdouble) + val.astype(np.longdouble)).astype(dt)
    assert ((two != one) & (z < 0)).any(), "the data can tell a contracted score from a rounded one"
    A, At = _handles(rp, ci, G.NROW, G.NCOL, val)
    Av, Atv = _handles(rp, ci, G.NROW, G.NCOL)
    for H, dv in ((1, 5), (3, G.widths(dtype)[2])):
        el, er, V, dO = _dev(gpu, *G.operands(dtype, H, dv, 3.0, 5))
        _pin_by_values(gpu, dtype, rp, ci, G.NROW, G.NCOL, A, At, Av, Atv, el, er, V, dO, H, 0.2, val)
    for h in (A, At, Av, Atv):
        h.free()


# ---- the bound --------------------------------------------------------------------------------------------------------

def _ratios(got, ref, what):
    r = G.ratios({k: v.cpu().numpy() for k, v in got.items()}, ref)
    print("%s: worst |got - ref| / bound  %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) <= 1, (what, r)
    return r


@pytest.mark.parametrize("dtype", DTYPES)
def test_inside_the_bound(crp, gpu, dtype):
    """every output of every (H, dv) of gat_ref.bound_cases against the np.longdouble reference, at two scales of the scores; the
    steep rows of DESIGN.md 5j (ascending, descending, late peak, half masked; T up to 60) with bias = 1; the second V block"""
    from crp_spmm_amd import hip
    rp, ci = G.matrix()
    A, At = _handles(rp, ci, G.NROW, G.NCOL)
    for dt_, H, dv, spread in G.bound_cases():
        if dt_ != dtype:
            continue
        _, _, el, er, V, dO, ref = G.case(dtype, H, dv, spread)
        el, er, V, dO = _dev(gpu, el, er, V, dO)
        _ratios(_gat(A, At, gpu, el, er, V, dO, H, G.SLOPE), ref, (dtype, "H = %d, dv = %d, spread %g" % (H, dv, spread)))
    A.free()
    At.free()
    rp, ci, val, el, er, V, dO, ref = G.steep_case(dtype)
    A, At = _handles(rp, ci, rp.size - 1, 80, val)
    el, er, V, dO = _dev(gpu, el, er, V, dO)
    got = _gat(A, At, gpu, el, er, V, dO, el.shape[1], G.SLOPE, bias=True)
    _ratios(got, ref, (dtype, "steep rows with bias"))
    masked = np.flatnonzero(~np.isfinite(val))
    assert masked.size and bool((got["p"][masked] == 0).all()) and bool((got["ds"][masked] == 0).all())
    A.free()
    At.free()
    rp, ci, el, er, V, ref = G.second_block_case(dtype)
    A = hip.CsrDev(rp.size - 1, G.NCOL, rp, ci, np.ones(ci.size))
    el, er, V = _dev(gpu, el, er, V)
    _ratios(_gat(A, None, gpu, el, er, V, None, 1, G.SLOPE, backward=False), ref, (dtype, "second V block, dv = %d" % V.shape[1]))
    A.free()


# ---- invariance -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_invariance(crp, gpu, dtype):
    """repeated calls; with and without the optional outputs; offset pointers and odd leading dimensions (the element path against
    the 16-byte path); two sources against one; a row-subset pair against the full handle; head h of an H-head call against the
    one-head call on head h's column views -- all bit for bit"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.matrix()
    nrow, ncol, nnz = G.NROW, G.NCOL, ci.size
    rows = R.rows_of(rp)
    val = np.random.default_rng(3).standard_normal(nnz)
    A, At = _handles(rp, ci, nrow, ncol, val)
    H = 3
    w = G.W[dtype]
    for dv in (8 * w, 32 * w + w):
        eln, ern, Vn, dOn = G.operands(dtype, H, dv, 2.0, 31)
        el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
        want = _gat(A, At, gpu, el, er, V, dO, H, 0.2, bias=True)
        _same(_gat(A, At, gpu, el, er, V, dO, H, 0.2, bias=True), want, (dtype, dv, "a repeated call"))
        # without the optional outputs
        O = A.gat_attention(el, er, V, slope=0.2, bias=True, heads=H)
        d_el, delta = A.gat_attention_bwd_row(el, er, V, want["O"], dO, want["lse"], slope=0.2, bias=True, heads=H)
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
            A.gat_attention(sel, ser, sV, slope=0.2, bias=True, out=O, lse=lse, p_out=p, heads=H)
            A.gat_attention_bwd_row(sel, ser, sV, O, sdO, lse, slope=0.2, bias=True, d_el=d_el, delta=delta, ds_out=ds, heads=H)
            At.gat_attention_bwd_col(ser, sV, sel, sdO, lse, delta, slope=0.2, bias=True, d_er=d_er, dV=dV, heads=H)
            torch.cuda.synchronize()
            got = dict(O=O.contiguous(), lse=lse, p=p, delta=delta, ds=ds, d_el=d_el.contiguous(), d_er=d_er.contiguous(), dV=dV.contiguous())
            _same(got, want, (dtype, dv, "ld + %d, offset %d" % (ld_extra, off)))
        # dV is V on the column side
        Vc = V.clone()
        d_er, dV = At.gat_attention_bwd_col(er, Vc, el, dO, want["lse"], want["delta"], slope=0.2, bias=True, dV=Vc, heads=H)
        torch.cuda.synchronize()
        assert dV is Vc
        _same(dict(d_er=d_er, dV=dV), want, (dtype, dv, "dV is V"))
        # two sources
        A2 = hip.CsrDev(nrow, G.K0, rp, G.two_source_codes(ci), val)
        got = _gat(A2, None, gpu, el, er[:G.K0], V[:G.K0], dO, H, 0.2, bias=True, er1=er[G.K0:], V1=V[G.K0:])
        _same(got, want, (dtype, dv, "two sources"))
        A2.free()
        # a row-subset pair with row maps, writing one set of outputs through its positions
        O, d_el = _nan(gpu, V, nrow, H * dv), _nan(gpu, V, nrow, H)
        lse, delta, p, ds = _nan(gpu, V, nrow, H), _nan(gpu, V, nrow, H), _nan(gpu, V, nnz, H), _nan(gpu, V, nnz, H)
        pick = (np.arange(nrow) % 4) % 3 == 0
        for sel in (pick, ~pick):
            r = np.flatnonzero(sel)
            keep = sel[rows]
            h = hip.CsrDev(r.size, ncol, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], val[keep])
            h.set_rowmap(r, nrow)
            pos = torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)
            h.gat_attention(el, er, V, slope=0.2, bias=True, out=O, lse=lse, p_out=p, out_pos=pos, heads=H)
            h.gat_attention_bwd_row(el, er, V, O, dO, lse, slope=0.2, bias=True, d_el=d_el, delta=delta, ds_out=ds, out_pos=pos, heads=H)
            torch.cuda.synchronize()
            h.free()
        _same(dict(O=O, lse=lse, p=p, delta=delta, ds=ds, d_el=d_el), want, (dtype, dv, "row subsets"))
        # out_pos as a permutation
        perm = np.random.default_rng(2).permutation(nnz).astype(np.int32)
        pos = torch.from_numpy(perm).to(gpu)
        lse, p, ds = _nan(gpu, V, nrow, H), _nan(gpu, V, nnz, H), _nan(gpu, V, nnz, H)
        O = A.gat_attention(el, er, V, slope=0.2, bias=True, lse=lse, p_out=p, out_pos=pos, heads=H)
        A.gat_attention_bwd_row(el, er, V, O, dO, lse, slope=0.2, bias=True, ds_out=ds, out_pos=pos, heads=H)
        torch.cuda.synchronize()
        idx = torch.from_numpy(perm.astype(np.int64)).to(gpu)
        assert torch.equal(p[idx], want["p"]) and torch.equal(ds[idx], want["ds"]), (dtype, dv, "out_pos as a permutation")
        # head h of the H-head call against the one-head call on head h's column views
        for h in range(H):
            sv = slice(h * dv, (h + 1) * dv)
            one = _gat(A, At, gpu, el[:, h:h + 1], er[:, h:h + 1], V[:, sv], dO[:, sv], 1, 0.2, bias=True)
            mine = {k: (want[k][:, sv] if k in ("O", "dV") else want[k][:, h:h + 1]) for k in KEYS}
            _same(one, mine, (dtype, dv, "head %d against the one-head call" % h))
    A.free()
    At.free()


# ---- special cases ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_special_cases_and_sentinels(crp, gpu, dtype):
    """empty rows, one-entry rows, masked edges (a value of -inf; er = -inf with slope > 0), all-masked rows (values; el = -inf);
    sentinels around everything not named stay untouched; NaN in rows no entry names changes nothing"""
    import torch
    rp, ci = G.matrix()
    nrow, ncol, nnz = G.NROW, G.NCOL, ci.size
    rows = R.rows_of(rp)
    lens = np.diff(rp)
    H, dv = 3, 5
    val = np.random.default_rng(12).standard_normal(nnz)
    empty, one = np.flatnonzero(lens == 0), np.flatnonzero(lens == 1)
    assert empty.size >= 2 and one.size >= 1
    dead_row, dead_row2 = 3, 5                                        # rows of 8 and 17 entries
    dead_col = next(int(c) for c in ci[rp[6]:rp[7]] if c not in ci[rp[one]])      # a column the 70-entry row names, no one-entry row
    val[rp[dead_row]:rp[dead_row + 1]] = -np.inf
    val[rp[4] + 1] = -np.inf                                          # one masked edge in the 9-entry row
    eln, ern, Vn, dOn = G.operands(dtype, H, dv, 1.5, 61)
    eln, ern = eln.copy(), ern.copy()
    eln[dead_row2, 1] = -np.inf                                       # head 1 of that row: every z is -inf
    ern[dead_col, 2] = -np.inf                                        # head 2 of every edge into that column
    A, At = _handles(rp, ci, nrow, ncol, val)
    el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
    got = _gat(A, At, gpu, el, er, V, dO, H, 0.2, bias=True)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert (g["lse"][empty] == -np.inf).all() and (g["O"][empty] == 0).all() and not np.signbit(g["O"][empty]).any()
    assert (g["d_el"][empty] == 0).all() and np.array_equal(g["delta"][empty], np.zeros((empty.size, H)))
    for r in one:
        assert np.array_equal(g["O"][r], Vn[ci[rp[r]]]), "a one-entry row: O = V[c] bit for bit"
        assert (g["p"][rp[r]] == 1).all()
    assert (g["lse"][dead_row] == -np.inf).all() and (g["O"][dead_row] == 0).all() and (g["p"][rp[dead_row]:rp[dead_row + 1]] == 0).all()
    assert (g["ds"][rp[dead_row]:rp[dead_row + 1]] == 0).all() and (g["d_el"][dead_row] == 0).all()
    assert g["lse"][dead_row2, 1] == -np.inf and (g["O"][dead_row2, dv:2 * dv] == 0).all() and np.isfinite(g["lse"][dead_row2, [0, 2]]).all()
    assert (g["p"][rp[4] + 1] == 0).all() and (g["ds"][rp[4] + 1] == 0).all()
    into = np.flatnonzero(ci == dead_col)
    live = into[np.isfinite(val[into])]
    assert live.size and (g["p"][live, 2] == 0).all() and (g["p"][live, 0] > 0).all()
    assert (g["d_er"][dead_col, 2] == 0) and (g["dV"][dead_col, 2 * dv:] == 0).all() and np.abs(g["dV"][dead_col, :dv]).max() > 0
    assert (g["d_er"][G.EMPTY_COL] == 0).all() and (g["dV"][G.EMPTY_COL] == 0).all()
    assert all(np.isfinite(g[k]).all() for k in KEYS if k != "lse")
    # inside the bound as well: masked edges and rows are the reference's exact zeros
    _ratios(got, G.reference(rp, ci, eln, ern, Vn, 0.2, val, dOn), (dtype, "special cases"))
    # NaN where no entry looks: the er and V rows of a column nobody names, el of the empty rows
    eln2, ern2, Vn2 = eln.copy(), ern.copy(), Vn.copy()
    ern2[G.EMPTY_COL], Vn2[G.EMPTY_COL], eln2[empty] = np.nan, np.nan, np.nan
    el2, er2, V2 = _dev(gpu, eln2, ern2, Vn2)
    again = _gat(A, At, gpu, el2, er2, V2, dO, H, 0.2, bias=True)
    _same(again, got, (dtype, "NaN in rows no entry names"))
    # sentinels: pad columns of O / dV / d_el / d_er, the tails of lse / p_out / delta / ds_out
    pad = 3
    mk = lambda r, c: torch.full((r, c), SENT, dtype=V.dtype, device=gpu)
    O, dV, d_el, d_er = mk(nrow + 1, H * dv + pad), mk(ncol + 1, H * dv + pad), mk(nrow + 1, H + pad), mk(ncol + 1, H + pad)
    lse, delta, p, ds = mk(nrow + 1, H), mk(nrow + 1, H), mk(nnz + 1, H), mk(nnz + 1, H)
    A.gat_attention(el, er, V, slope=0.2, bias=True, out=O[:nrow, :H * dv], lse=lse, p_out=p, heads=H)
    A.gat_attention_bwd_row(el, er, V, got["O"], dO, got["lse"], slope=0.2, bias=True, d_el=d_el[:nrow, :H], delta=delta, ds_out=ds, heads=H)
    At.gat_attention_bwd_col(er, V, el, dO, got["lse"], got["delta"], slope=0.2, bias=True, d_er=d_er[:ncol, :H], dV=dV[:ncol, :H * dv], heads=H)
    torch.cuda.synchronize()
    for t, r, c, k in ((O, nrow, H * dv, "O"), (dV, ncol, H * dv, "dV"), (d_el, nrow, H, "d_el"), (d_er, ncol, H, "d_er"), (lse, nrow, H, "lse"),
                       (delta, nrow, H, "delta"), (p, nnz, H, "p"), (ds, nnz, H, "ds")):
        assert torch.equal(t[:r, :c], got[k]), k
        assert bool((t[r:] == SENT).all()) and bool((t[:, c:] == SENT).all()), (k, "a sentinel was overwritten")
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_error_codes_that_need_a_live_handle(crp, gpu, dtype):
    """-4 for a leading dimension below its width, -1 for heads < 1, dv < 1, a bias other than 0 or 1, a non-finite slope, a NULL
    required pointer and the column side on a handle with negative codes; CRP_ATTN_BWD_EWIDTH for a head over the cap on both
    sides of the backward -- all with nothing written; the forward serves that width"""
    import torch
    from crp_spmm_amd import hip
    lib = crp.load()
    tdt = _tdt(dtype)
    sfx = "f64" if dtype == "float64" else "f32"
    cap = B.CAP[np.dtype(dtype)]
    rp, ci = G.matrix()
    nrow, ncol, nnz = 12, G.NCOL, int(rp[12])
    rp, ci = rp[:13], ci[:nnz]
    A, At = _handles(rp, ci, nrow, ncol)
    ffw, frow, fcol = (getattr(lib, "crp_gat_attention_%scsr_%s" % (k, sfx)) for k in ("", "bwd_row_", "bwd_col_"))
    P = lambda t: t.data_ptr()

    def calls(H, dv, told=None, ldel=None, ldv=None, slope=0.2, bias=0, null=False, col_handle=None):
        wv = H * dv
        th, tdv = told if told is not None else (H, dv)
        ldel, ldv = (H if ldel is None else ldel), (wv if ldv is None else ldv)
        el, er, V, O = (torch.ones(s, dtype=tdt, device=gpu) for s in ((nrow, H), (ncol, H), (ncol, wv), (nrow, wv)))
        lse_in = torch.zeros((nrow, H), dtype=tdt, device=gpu)
        outs = [torch.full(s, SENT, dtype=tdt, device=gpu) for s in ((nrow, wv), (nrow, H), (nnz, H), (nrow, H), (nrow, H), (nnz, H), (ncol, H),
                                                                      (ncol, wv))]
        Oo, lse, p, d_el, delta, ds, d_er, dV = outs
        elp = None if null else P(el)
        rcs = (ffw(A.handle, th, tdv, slope, bias, elp, ldel, P(er), H, None, 0, P(V), ldv, None, 0, P(Oo), wv, P(lse), P(p), None, None),
               frow(A.handle, th, tdv, slope, bias, elp, ldel, P(er), H, None, 0, P(V), ldv, None, 0, P(O), wv, P(O), wv, P(lse_in), P(d_el), H,
                    P(delta), P(ds), None, None),
               fcol((col_handle or At).handle, th, tdv, slope, bias, P(er), H, P(V), ldv, elp, ldel, P(O), wv, P(lse_in), P(lse_in), P(d_er), H,
                    P(dV), wv, None))
        torch.cuda.synchronize()
        return rcs, outs
    untouched = lambda outs: all(bool((t == SENT).all()) for t in outs)
    for kw in (dict(ldel=1), dict(ldv=15)):
        rcs, outs = calls(2, 8, **kw)
        assert rcs == (-4, -4, -4) and untouched(outs), (kw, rcs)
    for kw in (dict(told=(0, 8)), dict(told=(-2, 8)), dict(told=(2, 0)), dict(bias=2), dict(slope=float("nan")), dict(slope=float("inf")),
               dict(null=True)):
        rcs, outs = calls(2, 8, **kw)
        assert rcs == (-1, -1, -1) and untouched(outs), (kw, rcs)
    A2 = hip.CsrDev(nrow, G.K0, rp, G.two_source_codes(ci), np.ones(nnz))
    rcs, outs = calls(2, 8, col_handle=A2)                             # (as a column handle: its codes name a second source)
    assert rcs[2] == -1 and untouched(outs[6:]), rcs
    A2.free()
    rcs, outs = calls(2, 8)
    assert rcs == (0, 0, 0) and not any(bool((t == SENT).any()) for t in outs), rcs
    rcs, outs = calls(1, cap + G.W[dtype])                            # (the forward has no cap)
    assert rcs[0] == 0 and rcs[1:] == (B.EWIDTH, B.EWIDTH) and untouched(outs[3:]) and not bool((outs[0] == SENT).any()), rcs
    A.free()
    At.free()


# ---- hip.gat_attention ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_gat_attention_function_against_autograd(crp, gpu, dtype):
    """the gradients of el, er and V through hip.gat_attention against torch autograd on an index-based fp64 formulation (gather,
    leaky_relu, a scatter softmax, index_add), within the sum of the two computations' bounds (in the operands' dtype
    and in fp64)"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.matrix()
    nrow, ncol, nnz = G.NROW, G.NCOL, ci.size
    H, dv, slope = 3, 5, 0.2
    A, At = _handles(rp, ci, nrow, ncol)
    eln, ern, Vn, dOn = G.operands(dtype, H, dv, 1.5, 17)
    ref = G.reference(rp, ci, eln, ern, Vn, slope, None, dOn)
    ref64 = G.reference(rp, ci, *(x.astype(np.float64) for x in (eln, ern, Vn)), float(np.dtype(dtype).type(slope)), None, dOn.astype(np.float64))
    el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
    elg, erg, Vg = (t.clone().requires_grad_(True) for t in (el, er, V))
    O = hip.gat_attention(A, At, elg, erg, Vg, slope=slope, heads=H)
    O.backward(dO)
    torch.cuda.synchronize()
    # the same function from indexing primitives, in fp64 on the dtype-rounded data (and the dtype-rounded slope)
    ri = torch.from_numpy(R.rows_of(rp).astype(np.int64)).to(gpu)
    cj = torch.from_numpy(ci.astype(np.int64)).to(gpu)
    e2, r2, V2 = (t.double().clone().requires_grad_(True) for t in (el, er, V))
    s = torch.nn.functional.leaky_relu(e2[ri] + r2[cj], float(np.dtype(dtype).type(slope)))
    m = torch.full((nrow, H), float("-inf"), dtype=torch.float64, device=gpu).scatter_reduce(0, ri[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - m[ri].detach())
    den = torch.zeros((nrow, H), dtype=torch.float64, device=gpu).index_add(0, ri, ex)
    prob = ex / den[ri]
    O2 = torch.zeros((nrow, H, dv), dtype=torch.float64, device=gpu).index_add(0, ri, prob[:, :, None] * V2[cj].view(nnz, H, dv)).view(nrow, H * dv)
    O2.backward(dO.double())
    torch.cuda.synchronize()
    for k, mine, theirs in (("O", O.detach(), O2.detach()), ("d_el", elg.grad, e2.grad), ("d_er", erg.grad, r2.grad), ("dV", Vg.grad, V2.grad)):
        tol = (ref[k][1] + ref64[k][1]).astype(np.float64)
        err = np.abs(mine.double().cpu().numpy() - theirs.cpu().numpy())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0))
        print("%s %s: worst |hip - autograd| / (sum of the bounds) %.3g" % (dtype, k, ratio.max()))
        assert ratio.max() <= 1, (dtype, k, float(ratio.max()))
    A.free()
    At.free()
