"""GPU: the fused GATv2 attention and its two-handle backward (crp_gatv2_attention_csr_*, crp_gatv2_attention_bwd_row_csr_*,
crp_gatv2_attention_bwd_col_csr_*, crp_col_sum_*, the CsrDev wrappers, hip.col_sum and hip.gatv2_attention).

Bit pins against the kernels that exist (torch.equal, no tolerance, nothing compared with the code under test):
  XT = 0, slope = 1  r = fl(0 + xs) = xs on data without -0, so the score is the SDDMM's dot of a with XS[c]: O, lse, p_out equal
                     attention(heads = H, dk = dv, Q = a in every row, K = V = XS, scale = 1), delta and ds_out its
                     attention_bwd_q's, da_part its dQ, and dXS = dK + dV of attention_bwd_kv, added once in the dtype;
  dv = 1, a = 1      the score is lrelu(fl(xt + xs)): forward, delta and ds_out equal gat_attention(el = XT, er = XS, V = XS) and
                     its row side, for slopes 0.2, 0.25 and 0;
  exact data         small integers under power-of-two scales make every z, r, product and partial sum exact, so numpy's score has
                     the kernel's bits whatever the order: per head, the single-head attention with Q = 0, bias = 1 on a handle
                     whose values are those scores -- with and without the call's own bias;
  col_sum            numpy's replay of the order (pure additions).
Then everything inside the bound of DESIGN.md 5p against tests/gatv2_ref.reference, the invariances, the special cases, the error
codes and hip.gatv2_attention against torch autograd.  Pattern: gat_ref.matrix(), 40 x 80 with rows of 0, 1, 7, 8, 9, 17 and 70
entries; the cap runs on its rows of at most 9 entries."""
import numpy as np
import pytest

import attention_ref as R
import gatv2_ref as G2
from test_gpu_attention import SENT, _strided, _tdt

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
KEYS = G2.FWD_KEYS + G2.BWD_KEYS
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


def _g2(A, At, gpu, XT, XS, a, dO, H, slope, bias=False, XS1=None, backward=True):
    """one forward, row side, col_sum and (At given) column side -> dict of device tensors, every output asked for"""
    import torch
    from crp_spmm_amd import hip
    nrow, nnz = XT.shape[0], A.nnz
    lse, p = _nan(gpu, XT, nrow, H), _nan(gpu, XT, nnz, H)
    O = A.gatv2_attention(XT, XS, a, XS1=XS1, slope=slope, bias=bias, lse=lse, p_out=p, heads=H)
    out = dict(O=O, lse=lse, p=p)
    if backward:
        ds = _nan(gpu, XT, nnz, H)
        dXT, da_part, delta = A.gatv2_attention_bwd_row(XT, XS, a, O, dO, lse, XS1=XS1, slope=slope, bias=bias, ds_out=ds, heads=H)
        out.update(delta=delta, ds=ds, dXT=dXT, da_part=da_part, da=hip.col_sum(da_part))
        if At is not None:
            out.update(dXS=At.gatv2_attention_bwd_col(XS, XT, a, dO, lse, delta, slope=slope, bias=bias, heads=H))
    torch.cuda.synchronize()
    return out


def _same(got, want, what, keys=KEYS):
    import torch
    for k in keys:
        if k in got and k in want:
            assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
            assert torch.equal(got[k], want[k]), (what, k, "differs")


def _cases(dtype):
    for i, dv in enumerate(G2.widths(dtype)):
        for H in (1, 3):
            yield i, H, dv


def _finite(got):
    return all(bool(got[k].isfinite().all()) for k in got if k != "lse")


# ---- bit pins ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_xt_zero_slope_one_equals_the_attention_with_q_equal_a(crp, gpu, dtype):
    import torch
    full = G2.matrix()
    short = G2.short_matrix()[:2]
    val = {id(full): np.random.default_rng(8).standard_normal(full[1].size), id(short): np.random.default_rng(9).standard_normal(short[1].size)}
    hs = {id(m): _handles(m[0], m[1], m[0].size - 1, G2.NCOL, val[id(m)]) for m in (full, short)}
    cases = [(i, H, dv, full) for i, H, dv in _cases(dtype)] + [(9, 1, G2.cap(dtype), short), (10, 3, G2.cap(dtype) // 2 + G2.W[dtype], short)]
    for i, H, dv, m in cases:
        (rp, ci), (A, At) = m, hs[id(m)]
        nrow = rp.size - 1
        _, XSn, an, dOn = G2.operands(dtype, H, dv, 2.0, 50 + i, nrow=nrow)
        assert not np.signbit(XSn[XSn == 0]).any()
        XS, a, dO = _dev(gpu, XSn, an, dOn)
        XT = torch.zeros((nrow, H * dv), dtype=XS.dtype, device=gpu)
        Q = a.reshape(1, -1).repeat(nrow, 1).contiguous()
        flat = (lambda t: t.view(-1)) if H == 1 else (lambda t: t)
        for bias in (False, True):
            lse, p, ds = _nan(gpu, XS, nrow, H), _nan(gpu, XS, ci.size, H), _nan(gpu, XS, ci.size, H)
            O = A.attention(Q, XS, XS, scale=1.0, bias=bias, lse=flat(lse), p_out=flat(p), heads=H)
            dQ, delta = A.attention_bwd_q(Q, XS, XS, O, dO, flat(lse), scale=1.0, bias=bias, ds_out=flat(ds), heads=H)
            dK, dV = At.attention_bwd_kv(XS, XS, Q, dO, flat(lse), flat(delta), scale=1.0, bias=bias, heads=H)
            torch.cuda.synchronize()
            want = dict(O=O, lse=lse, p=p, delta=delta.view(nrow, H), ds=ds, da_part=dQ, dXS=dK + dV)
            got = _g2(A, At, gpu, XT, XS, a, dO, H, 1.0, bias=bias)
            _same(got, want, (dtype, H, dv, "bias" if bias else "no bias"))
            assert _finite(got)
    for A, At in hs.values():
        A.free()
        At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_column_and_a_equal_one_is_the_gat_score(crp, gpu, dtype):
    import torch
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
    val = np.random.default_rng(18).standard_normal(nnz)
    A, At = _handles(rp, ci, nrow, ncol, val)
    for H in (1, 3):
        XTn, XSn, _, dOn = G2.operands(dtype, H, 1, 1.0, 40 + H)
        XT, XS, dO = _dev(gpu, 2 * XTn, 2 * XSn, dOn)
        a = torch.ones(H, dtype=XT.dtype, device=gpu)
        for slope in SLOPES:
            for bias in (False, True):
                lse, p, ds = _nan(gpu, XT, nrow, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nnz, H)
                O = A.gat_attention(XT, XS, XS, slope=slope, bias=bias, lse=lse, p_out=p, heads=H)
                _, delta = A.gat_attention_bwd_row(XT, XS, XS, O, dO, lse, slope=slope, bias=bias, ds_out=ds, heads=H)
                torch.cuda.synchronize()
                got = _g2(A, At, gpu, XT, XS, a, dO, H, slope, bias=bias)
                _same(got, dict(O=O, lse=lse, p=p, delta=delta, ds=ds), (dtype, H, slope, bias))
                assert _finite(got)
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_any_width_and_slope_on_exact_data_equals_the_attention_on_scores_as_values(crp, gpu, dtype):
    import torch
    dt = np.dtype(dtype)
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
    val = np.random.default_rng(4).integers(-4, 5, nnz).astype(np.float64)
    A0, At0 = _handles(rp, ci, nrow, ncol)
    A1, At1 = _handles(rp, ci, nrow, ncol, val)
    from crp_spmm_amd import hip
    Av = hip.CsrDev(nrow, ncol, rp, ci, np.ones(nnz))
    Q0 = torch.zeros((nrow, 1), dtype=_tdt(dtype), device=gpu)
    K0 = torch.zeros((ncol, 1), dtype=_tdt(dtype), device=gpu)
    for i, H, dv in _cases(dtype):
        XTn, XSn, an, dOn = G2.exact_operands(dtype, H, dv, 90 + i)
        XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
        for (A, At), v in (((A0, At0), None), ((A1, At1), val)):
            got = _g2(A, At, gpu, XT, XS, a, dO, H, 0.25, bias=v is not None)
            for h in range(H):
                s, z, r = G2.scores_dtype(rp, ci, XTn, XSn, an, 0.25, h, v)
                exact = G2.scores_exact(rp, ci, XTn, XSn, an, 0.25, h, v)[0]
                assert np.array_equal(s.astype(np.longdouble), exact), "every step of the score is exact on this data"
                Av.update_values(s.astype(np.float64))
                sv = slice(h * dv, (h + 1) * dv)
                lse, p, ds = _nan(gpu, XT, nrow), _nan(gpu, XT, nnz), _nan(gpu, XT, nnz)
                O = Av.attention(Q0, K0, XS[:, sv], scale=1.0, bias=True, lse=lse, p_out=p)
                _, delta = Av.attention_bwd_q(Q0, K0, XS[:, sv], O, dO[:, sv], lse, scale=1.0, bias=True, ds_out=ds)
                torch.cuda.synchronize()
                mine = dict(O=got["O"][:, sv], lse=got["lse"][:, h], p=got["p"][:, h], delta=got["delta"][:, h], ds=got["ds"][:, h])
                _same(mine, dict(O=O, lse=lse, p=p, delta=delta, ds=ds), (dtype, "H = %d, dv = %d, head %d, bias %s" % (H, dv, h, v is not None)))
            assert _finite(got) and dt == XTn.dtype
    for h in (A0, At0, A1, At1, Av):
        h.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_col_sum_equals_the_replay(crp, gpu, dtype):
    import torch
    from crp_spmm_amd import hip
    rng = np.random.default_rng(21)
    for nrow, n in ((0, 5), (1, 1), (255, 3), (256, 8), (257, 33), (600, 7), (1030, 300)):
        x = rng.standard_normal((nrow, n)).astype(dtype)
        want = _dev(gpu, G2.col_sum_replay(x))[0]
        assert torch.equal(hip.col_sum(_dev(gpu, x)[0]), want), (nrow, n)
        for ld_extra, off in ((1, 1), (4, 0), (3, 2)):
            out = torch.full((n + 2,), SENT, dtype=want.dtype, device=gpu)
            hip.col_sum(_strided(gpu, x, n + ld_extra, off), out=out[:n])
            torch.cuda.synchronize()
            assert torch.equal(out[:n], want) and bool((out[n:] == SENT).all()), (nrow, n, ld_extra, off)


# ---- the bound --------------------------------------------------------------------------------------------------------

def _ratios(got, ref, what):
    r = G2.ratios({k: v.cpu().numpy() for k, v in got.items()}, ref)
    print("%s: worst |got - ref| / bound  %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) <= 1, (what, r)
    return r


@pytest.mark.parametrize("dtype", DTYPES)
def test_inside_the_bound(crp, gpu, dtype):
    """every output of every (H, dv) of gatv2_ref.bound_cases against the np.longdouble reference, at two scales of the scores, the
    cap on the short rows; the steep rows of DESIGN.md 5j (ascending, descending, late peak, half masked; T up to 60) with bias = 1"""
    rp, ci = G2.matrix()
    rps, cis, _ = G2.short_matrix()
    hs = {False: _handles(rp, ci, G2.NROW, G2.NCOL), True: _handles(rps, cis, rps.size - 1, G2.NCOL)}
    for dt_, H, dv, spread, short in G2.bound_cases():
        if dt_ != dtype:
            continue
        _, _, XT, XS, a, dO, ref = G2.case(dtype, H, dv, spread, short)
        XT, XS, a, dO = _dev(gpu, XT, XS, a, dO)
        _ratios(_g2(*hs[short], gpu, XT, XS, a, dO, H, G2.SLOPE), ref, (dtype, "H = %d, dv = %d, spread %g" % (H, dv, spread)))
    for A, At in hs.values():
        A.free()
        At.free()
    rp, ci, val, XT, XS, a, dO, ref = G2.steep_case(dtype)
    A, At = _handles(rp, ci, rp.size - 1, 80, val)
    XT, XS, a, dO = _dev(gpu, XT, XS, a, dO)
    got = _g2(A, At, gpu, XT, XS, a, dO, a.shape[0], G2.SLOPE, bias=True)
    _ratios(got, ref, (dtype, "steep rows with bias"))
    masked = np.flatnonzero(~np.isfinite(val))
    assert masked.size and bool((got["p"][masked] == 0).all()) and bool((got["ds"][masked] == 0).all())
    A.free()
    At.free()


# ---- invariance -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_invariance(crp, gpu, dtype):
    """repeated calls; with and without the optional outputs; offset pointers and odd leading dimensions (the element path against
    the 16-byte path); dXS is XS; two sources against one; a row-subset pair against the full handle; out_pos as a permutation;
    head h of an H-head call against the one-head call on head h's column views -- all bit for bit"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
    rows = R.rows_of(rp)
    val = np.random.default_rng(3).standard_normal(nnz)
    A, At = _handles(rp, ci, nrow, ncol, val)
    H = 3
    w = G2.W[dtype]
    kw = dict(slope=0.2, bias=True, heads=H)
    for dv in (8 * w, 32 * w + w, 64 * w + w):
        XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 2.0, 31)
        XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
        want = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, bias=True)
        _same(_g2(A, At, gpu, XT, XS, a, dO, H, 0.2, bias=True), want, (dtype, dv, "a repeated call"))
        # without the optional outputs
        O = A.gatv2_attention(XT, XS, a, **kw)
        dXT, da_part, delta = A.gatv2_attention_bwd_row(XT, XS, a, want["O"], dO, want["lse"], **kw)
        torch.cuda.synchronize()
        _same(dict(O=O, dXT=dXT, da_part=da_part, delta=delta), want, (dtype, dv, "without the optional outputs"))
        # offset pointers and odd leading dimensions
        for ld_extra, off in ((1, 0), (0, 1), (3, 1)):
            sXT, sXS, sdO = (_strided(gpu, t, t.shape[1] + ld_extra, off) for t in (XTn, XSn, dOn))
            sa = _strided(gpu, an.reshape(1, -1), H * dv, off)[0]
            mk = lambda r: _strided(gpu, np.zeros((r, H * dv), dtype), H * dv + ld_extra, off)
            O, dXT, da_part, dXS = mk(nrow), mk(nrow), mk(nrow), mk(ncol)
            lse, p, ds, delta = _nan(gpu, XT, nrow, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nrow, H)
            A.gatv2_attention(sXT, sXS, sa, out=O, lse=lse, p_out=p, **kw)
            A.gatv2_attention_bwd_row(sXT, sXS, sa, O, sdO, lse, dXT=dXT, da_part=da_part, delta=delta, ds_out=ds, **kw)
            At.gatv2_attention_bwd_col(sXS, sXT, sa, sdO, lse, delta, dXS=dXS, **kw)
            da = hip.col_sum(da_part)
            torch.cuda.synchronize()
            got = dict(O=O.contiguous(), lse=lse, p=p, delta=delta, ds=ds, dXT=dXT.contiguous(), da_part=da_part.contiguous(),
                       dXS=dXS.contiguous(), da=da)
            _same(got, want, (dtype, dv, "ld + %d, offset %d" % (ld_extra, off)))
        # dXS is XS on the column side
        Xc = XS.clone()
        dXS = At.gatv2_attention_bwd_col(Xc, XT, a, dO, want["lse"], want["delta"], dXS=Xc, **kw)
        torch.cuda.synchronize()
        assert dXS is Xc
        _same(dict(dXS=dXS), want, (dtype, dv, "dXS is XS"))
        # two sources
        A2 = hip.CsrDev(nrow, G2.K0, rp, G2.two_source_codes(ci), val)
        got = _g2(A2, None, gpu, XT, XS[:G2.K0], a, dO, H, 0.2, bias=True, XS1=XS[G2.K0:])
        _same(got, want, (dtype, dv, "two sources"))
        A2.free()
        # a row-subset pair with row maps, writing one set of outputs through its positions
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
        # out_pos as a permutation
        perm = np.random.default_rng(2).permutation(nnz).astype(np.int32)
        pos = torch.from_numpy(perm).to(gpu)
        lse, p, ds = _nan(gpu, XT, nrow, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nnz, H)
        O = A.gatv2_attention(XT, XS, a, lse=lse, p_out=p, out_pos=pos, **kw)
        A.gatv2_attention_bwd_row(XT, XS, a, O, dO, lse, ds_out=ds, out_pos=pos, **kw)
        torch.cuda.synchronize()
        idx = torch.from_numpy(perm.astype(np.int64)).to(gpu)
        assert torch.equal(p[idx], want["p"]) and torch.equal(ds[idx], want["ds"]), (dtype, dv, "out_pos as a permutation")
        # head h of the H-head call against the one-head call on head h's column views
        for h in range(H):
            sv = slice(h * dv, (h + 1) * dv)
            one = _g2(A, At, gpu, XT[:, sv], XS[:, sv], a[h].clone(), dO[:, sv], 1, 0.2, bias=True)
            mine = {k: (want[k][sv] if k == "da" else want[k][:, sv] if k in ("O", "dXT", "da_part", "dXS") else want[k][:, h:h + 1])
                    for k in KEYS}
            _same(one, mine, (dtype, dv, "head %d against the one-head call" % h))
    A.free()
    At.free()


# ---- special cases ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_special_cases_and_sentinels(crp, gpu, dtype):
    """empty rows, one-entry rows, masked edges and an all-masked row (values of -inf); sentinels around everything not named stay
    untouched; NaN in rows no entry names changes nothing"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
    lens = np.diff(rp)
    H, dv = 3, 5
    wv = H * dv
    val = np.random.default_rng(12).standard_normal(nnz)
    empty, one = np.flatnonzero(lens == 0), np.flatnonzero(lens == 1)
    assert empty.size >= 2 and one.size >= 1
    dead_row = 3                                                      # a row of 8 entries
    val[rp[dead_row]:rp[dead_row + 1]] = -np.inf
    val[rp[4] + 1] = -np.inf                                          # one masked edge in the 9-entry row
    XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 1.5, 61)
    A, At = _handles(rp, ci, nrow, ncol, val)
    XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
    got = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, bias=True)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert (g["lse"][empty] == -np.inf).all() and (g["O"][empty] == 0).all() and not np.signbit(g["O"][empty]).any()
    assert (g["dXT"][empty] == 0).all() and (g["da_part"][empty] == 0).all() and np.array_equal(g["delta"][empty], np.zeros((empty.size, H)))
    for r in one:
        assert np.array_equal(g["O"][r], XSn[ci[rp[r]]]), "a one-entry row: O = XS[c] bit for bit"
        assert (g["p"][rp[r]] == 1).all()
    dead = slice(rp[dead_row], rp[dead_row + 1])
    assert (g["lse"][dead_row] == -np.inf).all() and (g["O"][dead_row] == 0).all() and (g["p"][dead] == 0).all()
    assert (g["ds"][dead] == 0).all() and (g["dXT"][dead_row] == 0).all() and (g["da_part"][dead_row] == 0).all()
    assert (g["p"][rp[4] + 1] == 0).all() and (g["ds"][rp[4] + 1] == 0).all()
    assert (g["dXS"][G2.EMPTY_COL] == 0).all() and not np.signbit(g["dXS"][G2.EMPTY_COL]).any()
    assert all(np.isfinite(g[k]).all() for k in KEYS if k != "lse")
    # inside the bound as well: masked edges and rows are the reference's exact zeros
    _ratios(got, G2.reference(rp, ci, XTn, XSn, an, 0.2, val, dOn), (dtype, "special cases"))
    # NaN where no entry looks: the XS row of a column nobody names, XT of the empty rows
    XTn2, XSn2 = XTn.copy(), XSn.copy()
    XSn2[G2.EMPTY_COL], XTn2[empty] = np.nan, np.nan
    XT2, XS2 = _dev(gpu, XTn2, XSn2)
    again = _g2(A, At, gpu, XT2, XS2, a, dO, H, 0.2, bias=True)
    _same(again, got, (dtype, "NaN in rows no entry names"))
    # sentinels: pad columns of O / dXT / da_part / dXS, the tails of lse / p_out / delta / ds_out / da
    pad = 3
    mk = lambda r, c: torch.full((r, c), SENT, dtype=XT.dtype, device=gpu)
    O, dXT, dap, dXS = mk(nrow + 1, wv + pad), mk(nrow + 1, wv + pad), mk(nrow + 1, wv + pad), mk(ncol + 1, wv + pad)
    lse, delta, p, ds, da = mk(nrow + 1, H), mk(nrow + 1, H), mk(nnz + 1, H), mk(nnz + 1, H), mk(1, wv + pad)
    kw = dict(slope=0.2, bias=True, heads=H)
    A.gatv2_attention(XT, XS, a, out=O[:nrow, :wv], lse=lse, p_out=p, **kw)
    A.gatv2_attention_bwd_row(XT, XS, a, got["O"], dO, got["lse"], dXT=dXT[:nrow, :wv], da_part=dap[:nrow, :wv], delta=delta, ds_out=ds, **kw)
    At.gatv2_attention_bwd_col(XS, XT, a, dO, got["lse"], got["delta"], dXS=dXS[:ncol, :wv], **kw)
    hip.col_sum(dap[:nrow, :wv], out=da[0, :wv])
    torch.cuda.synchronize()
    for t, r, c, k in ((O, nrow, wv, "O"), (dXT, nrow, wv, "dXT"), (dap, nrow, wv, "da_part"), (dXS, ncol, wv, "dXS"), (lse, nrow, H, "lse"),
                       (delta, nrow, H, "delta"), (p, nnz, H, "p"), (ds, nnz, H, "ds")):
        assert torch.equal(t[:r, :c], got[k]), k
        assert bool((t[r:] == SENT).all()) and bool((t[:, c:] == SENT).all()), (k, "a sentinel was overwritten")
    assert torch.equal(da[0, :wv], got["da"]) and bool((da[0, wv:] == SENT).all())
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_error_codes_that_need_a_live_handle(crp, gpu, dtype):
    """-4 for a leading dimension below its width, -1 for heads < 1, dv < 1, a bias other than 0 or 1, a non-finite slope, a NULL
    required pointer and the column side on a handle with negative codes; CRP_GATV2_EWIDTH for a head over the cap in both
    directions -- all with nothing written; the cap itself is served"""
    import torch
    from crp_spmm_amd import hip
    lib = crp.load()
    tdt = _tdt(dtype)
    sfx = "f64" if dtype == "float64" else "f32"
    cap = G2.cap(dtype)
    rp, ci = G2.matrix()
    nrow, ncol, nnz = 3, G2.NCOL, int(rp[3])
    rp, ci = rp[:4], ci[:nnz]
    A, At = _handles(rp, ci, nrow, ncol)
    ffw, frow, fcol = (getattr(lib, "crp_gatv2_attention_%scsr_%s" % (k, sfx)) for k in ("", "bwd_row_", "bwd_col_"))
    P = lambda t: t.data_ptr()

    def calls(H, dv, told=None, ldx=None, slope=0.2, bias=0, null=None, col_handle=None):
        wv = H * dv
        th, tdv = told if told is not None else (H, dv)
        ldx = wv if ldx is None else ldx
        XT, XS, O, a = (torch.ones(s, dtype=tdt, device=gpu) for s in ((nrow, wv), (ncol, wv), (nrow, wv), (wv,)))
        a /= wv                                                        # (scores of 2, whatever the width)
        lse_in = torch.zeros((nrow, H), dtype=tdt, device=gpu)
        outs = [torch.full(s, SENT, dtype=tdt, device=gpu) for s in ((nrow, wv), (nrow, H), (nnz, H), (nrow, wv), (nrow, wv), (nrow, H),
                                                                      (nnz, H), (ncol, wv))]
        Oo, lse, p, dXT, dap, delta, ds, dXS = outs
        xtp = None if null == "XT" else P(XT)
        ap = None if null == "a" else P(a)
        rcs = (ffw(A.handle, th, tdv, slope, bias, xtp, ldx, P(XS), wv, None, 0, ap, P(Oo), wv, P(lse), P(p), None, None),
               frow(A.handle, th, tdv, slope, bias, xtp, ldx, P(XS), wv, None, 0, ap, P(O), wv, P(O), wv, P(lse_in), P(dXT), wv, P(dap), wv,
                    P(delta), P(ds), None, None),
               fcol((col_handle or At).handle, th, tdv, slope, bias, P(XS), wv, xtp, ldx, ap, P(O), wv, P(lse_in), P(lse_in), P(dXS), wv, None))
        torch.cuda.synchronize()
        return rcs, outs
    untouched = lambda outs: all(bool((t == SENT).all()) for t in outs)
    rcs, outs = calls(2, 8, ldx=15)
    assert rcs == (-4, -4, -4) and untouched(outs), rcs
    for kw in (dict(told=(0, 8)), dict(told=(-2, 8)), dict(told=(2, 0)), dict(bias=2), dict(slope=float("nan")), dict(slope=float("inf")),
               dict(null="XT"), dict(null="a")):
        rcs, outs = calls(2, 8, **kw)
        assert rcs == (-1, -1, -1) and untouched(outs), (kw, rcs)
    A2 = hip.CsrDev(nrow, G2.K0, rp, G2.two_source_codes(ci), np.ones(nnz))
    rcs, outs = calls(2, 8, col_handle=A2)                             # (as a column handle: its codes name a second source)
    assert rcs[2] == -1 and untouched(outs[7:]), rcs
    A2.free()
    rcs, outs = calls(2, 8)
    assert rcs == (0, 0, 0) and not any(bool((t == SENT).any()) for t in outs), rcs
    rcs, outs = calls(1, cap)
    assert rcs == (0, 0, 0) and not any(bool((t == SENT).any()) for t in outs), rcs
    rcs, outs = calls(1, cap + 1)
    assert rcs == (G2.EWIDTH, G2.EWIDTH, G2.EWIDTH) and untouched(outs), rcs
    # ... and col_sum's
    fsum = getattr(lib, "crp_col_sum_" + sfx)
    x, work, out = torch.ones((4, 6), dtype=tdt, device=gpu), torch.full((6,), SENT, dtype=tdt, device=gpu), torch.full((6,), SENT, dtype=tdt, device=gpu)
    assert fsum(4, 6, P(x), 5, P(work), P(out), None) == -4
    assert fsum(-1, 6, P(x), 6, P(work), P(out), None) == -1 and fsum(4, -1, P(x), 6, P(work), P(out), None) == -1
    assert fsum(4, 6, None, 6, P(work), P(out), None) == -1 and fsum(4, 6, P(x), 6, None, P(out), None) == -1
    assert fsum(4, 6, P(x), 6, P(work), None, None) == -1
    torch.cuda.synchronize()
    assert untouched([work, out])
    assert fsum(4, 6, P(x), 6, P(work), P(out), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 4).all())
    A.free()
    At.free()


# ---- hip.gatv2_attention ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_gatv2_attention_function_against_autograd(crp, gpu, dtype):
    """the gradients of XT, XS and a through hip.gatv2_attention against torch autograd on an index-based fp64 formulation (gather,
    leaky_relu, a product with a, a scatter softmax, index_add), within the sum of the two computations' bounds (in
    the operands' dtype and in fp64)"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G2.matrix()
    nrow, ncol, nnz = G2.NROW, G2.NCOL, ci.size
    H, dv, slope = 3, 5, 0.2
    A, At = _handles(rp, ci, nrow, ncol)
    XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 1.5, 17)
    ref = G2.reference(rp, ci, XTn, XSn, an, slope, None, dOn)
    sl = float(np.dtype(dtype).type(slope))
    ref64 = G2.reference(rp, ci, *(x.astype(np.float64) for x in (XTn, XSn, an)), sl, None, dOn.astype(np.float64))
    XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
    XTg, XSg, ag = (t.clone().requires_grad_(True) for t in (XT, XS, a))
    O = hip.gatv2_attention(A, At, XTg, XSg, ag, slope=slope, heads=H)
    O.backward(dO)
    torch.cuda.synchronize()
    # the same function from indexing primitives, in fp64 on the dtype-rounded data (and the dtype-rounded slope)
    ri = torch.from_numpy(R.rows_of(rp).astype(np.int64)).to(gpu)
    cj = torch.from_numpy(ci.astype(np.int64)).to(gpu)
    T2, S2, a2 = (t.double().clone().requires_grad_(True) for t in (XT, XS, a))
    xs = S2[cj].view(nnz, H, dv)
    s = (torch.nn.functional.leaky_relu(T2[ri].view(nnz, H, dv) + xs, sl) * a2[None]).sum(dim=2)
    m = torch.full((nrow, H), float("-inf"), dtype=torch.float64, device=gpu).scatter_reduce(0, ri[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - m[ri].detach())
    den = torch.zeros((nrow, H), dtype=torch.float64, device=gpu).index_add(0, ri, ex)
    prob = ex / den[ri]
    O2 = torch.zeros((nrow, H, dv), dtype=torch.float64, device=gpu).index_add(0, ri, prob[:, :, None] * xs).view(nrow, H * dv)
    O2.backward(dO.double())
    torch.cuda.synchronize()
    assert ag.grad.shape == a.shape
    for k, mine, theirs in (("O", O.detach(), O2.detach()), ("dXT", XTg.grad, T2.grad), ("dXS", XSg.grad, S2.grad),
                            ("da", ag.grad.view(-1), a2.grad.view(-1))):
        tol = (ref[k][1] + ref64[k][1]).astype(np.float64)
        err = np.abs(mine.double().cpu().numpy() - theirs.cpu().numpy())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0))
        print("%s %s: worst |hip - autograd| / (sum of the bounds) %.3g" % (dtype, k, ratio.max()))
        assert ratio.max() <= 1, (dtype, k, float(ratio.max()))
    A.free()
    At.free()
