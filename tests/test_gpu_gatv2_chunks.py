"""GPU: the fused GATv2 attention, its two-handle backward and their dropout variants on gat_ref.chunk_matrix() -- rows of 0, 1, 7,
8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129 and 200 entries, the long ones in shuffled column order, a hub column of 277
entries and columns of exactly 0, 1, 8, 9, 63, 64 and 65: every edge of a chunk of LPR = 8, 16, 32 and 64 entries and up to five
chunks of 64, on the row side and on the column side -- at gatv2_ref.chunk_widths(): both sides of every threshold of the dispatch
table, the cap (P = 4, full, here on the long rows) and element-path widths inside the 32- and the 64-lane range.

The bound of DESIGN.md 5p is some 25 times what a correct kernel leaves, so on this pattern the bit pins are the sharp instrument.
Every output of the forward, the row side and the column side is held
  a. bit for bit against kernels that are pinned on such patterns themselves: XT = 0 and slope = 1 against the attention with
     Q = a and dk = dv at every width; dv = 1 and a = 1 against gat_attention; exact data against the attention on scores as values
     at one width per instance (test_gpu_gatv2.py);
  b. inside the bound of DESIGN.md 5p against the np.longdouble reference;
  c. under dropout: inside the bound of 5q at (DROP, SEED); dropout = 0 against the plain call; and, with XS = I and with a = 0 and
     dO = I, the dropped O and dXS against the plain call's, entry for entry -- which holds every keep bit of every chunk of the
     long rows and of the hub column (the mask itself: test_gpu_gat_chunks.py);
  d. against itself where the answer must not depend on the layout: two sources against one, head h of three against the one-head
     call, an odd leading dimension with an offset pointer (the element path) against the aligned call (the 16-byte path)."""
import numpy as np
import pytest

import dropout_ref as D
import gat_ref as G
import gatv2_ref as G2
from test_gpu_attention import _strided, _tdt
from test_gpu_gatv2 import KEYS, SLOPES, _dev, _finite, _g2, _handles, _nan, _ratios, _same
from test_gpu_gatv2_dropout import _g2 as _g2_drop
from test_gpu_gatv2_dropout import _ratios as _ratios_drop

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
NROW, NCOL, K0 = G.CHUNK_NROW, G.CHUNK_NCOL, G.CHUNK_K0


def _by_width(widths):
    """(dtype, dv) pairs as pytest parameters"""
    return [pytest.param(dtype, dv, id="%s-%d" % (dtype, dv)) for dtype in DTYPES for dv in widths(dtype)]


def _pin_widths(dtype):
    """every width of the chunk pattern and the widths of the 40 x 80 pattern, one or more per instance"""
    return tuple(sorted(set(G2.chunk_widths(dtype)) | set(G2.widths(dtype))))


def _exact_pin_widths(dtype):
    """one width per (LPR, P) of the table, 16-byte and element path in turn"""
    w = G2.W[dtype]
    out = (5, 16 * w, 17 * w + 1, 64 * w, 64 * w + 1, 256 * w)
    assert [G.instance_of("gatv2", dtype, dv) for dv in out] == [inst for _, inst in G.INSTANCES]
    return out


def _invariance_widths(dtype):
    """a 16-byte and an element-path width in the 32-lane range and in the P = 4 range"""
    w = G2.W[dtype]
    out = (32 * w, 17 * w + 1, 256 * w, 128 * w + 1)
    assert [G.instance_of("gatv2", dtype, dv) for dv in out] == [(32, 1), (32, 1), (64, 4), (64, 4)]
    return out


def _identity_heads(n, H, dt):
    return np.tile(np.eye(n, dtype=dt), (1, H))


# ---- a. bit pins ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dv", _by_width(_pin_widths))
def test_xt_zero_slope_one_equals_the_attention_with_q_equal_a(crp, gpu, dtype, dv):
    """r = fl(0 + xs) = xs, so the score is the SDDMM's dot of a with XS[c]: attention(heads = H, dk = dv, Q = a in every row,
    K = V = XS, scale = 1), its attention_bwd_q and dK + dV of its attention_bwd_kv (test_gpu_gatv2.py)"""
    import torch
    rp, ci = G.chunk_matrix()
    val = np.random.default_rng(8).standard_normal(ci.size)
    A, At = _handles(rp, ci, NROW, NCOL, val)
    for H in (1, 3):
        _, XSn, an, dOn = G2.operands(dtype, H, dv, 2.0, 50 + H, nrow=NROW, ncol=NCOL)
        assert not np.signbit(XSn[XSn == 0]).any()
        XS, a, dO = _dev(gpu, XSn, an, dOn)
        XT = torch.zeros((NROW, H * dv), dtype=XS.dtype, device=gpu)
        Q = a.reshape(1, -1).repeat(NROW, 1).contiguous()
        flat = (lambda t: t.view(-1)) if H == 1 else (lambda t: t)
        for bias in (False, True):
            lse, p, ds = _nan(gpu, XS, NROW, H), _nan(gpu, XS, ci.size, H), _nan(gpu, XS, ci.size, H)
            O = A.attention(Q, XS, XS, scale=1.0, bias=bias, lse=flat(lse), p_out=flat(p), heads=H)
            dQ, delta = A.attention_bwd_q(Q, XS, XS, O, dO, flat(lse), scale=1.0, bias=bias, ds_out=flat(ds), heads=H)
            dK, dV = At.attention_bwd_kv(XS, XS, Q, dO, flat(lse), flat(delta), scale=1.0, bias=bias, heads=H)
            torch.cuda.synchronize()
            want = dict(O=O, lse=lse, p=p, delta=delta.view(NROW, H), ds=ds, da_part=dQ, dXS=dK + dV)
            got = _g2(A, At, gpu, XT, XS, a, dO, H, 1.0, bias=bias)
            _same(got, want, (dtype, H, dv, "bias" if bias else "no bias"))
            assert _finite(got)
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_column_and_a_equal_one_is_the_gat_score(crp, gpu, dtype):
    """the score is lrelu(fl(xt + xs)): forward, delta and ds_out equal gat_attention(el = XT, er = XS, V = XS) and its row side"""
    import torch
    rp, ci = G.chunk_matrix()
    nnz = ci.size
    val = np.random.default_rng(18).standard_normal(nnz)
    A, At = _handles(rp, ci, NROW, NCOL, val)
    for H in (1, 3):
        XTn, XSn, _, dOn = G2.operands(dtype, H, 1, 1.0, 40 + H, nrow=NROW, ncol=NCOL)
        XT, XS, dO = _dev(gpu, 2 * XTn, 2 * XSn, dOn)
        a = torch.ones(H, dtype=XT.dtype, device=gpu)
        for slope in SLOPES:
            for bias in (False, True):
                lse, p, ds = _nan(gpu, XT, NROW, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nnz, H)
                O = A.gat_attention(XT, XS, XS, slope=slope, bias=bias, lse=lse, p_out=p, heads=H)
                _, delta = A.gat_attention_bwd_row(XT, XS, XS, O, dO, lse, slope=slope, bias=bias, ds_out=ds, heads=H)
                torch.cuda.synchronize()
                got = _g2(A, At, gpu, XT, XS, a, dO, H, slope, bias=bias)
                _same(got, dict(O=O, lse=lse, p=p, delta=delta, ds=ds), (dtype, H, slope, bias))
                assert _finite(got)
    A.free()
    At.free()


@pytest.mark.parametrize("dtype,dv", _by_width(_exact_pin_widths))
def test_exact_data_equals_the_attention_on_scores_as_values(crp, gpu, dtype, dv):
    """small integers under power-of-two scales make every z, r, product and partial sum exact, so numpy's score has the kernel's
    bits whatever the order: per head, the single-head attention with Q = 0, bias = 1 on a handle whose values are those scores,
    with and without the call's own bias (test_gpu_gatv2.py)"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.chunk_matrix()
    nnz = ci.size
    val = np.random.default_rng(4).integers(-4, 5, nnz).astype(np.float64)
    A0, At0 = _handles(rp, ci, NROW, NCOL)
    A1, At1 = _handles(rp, ci, NROW, NCOL, val)
    Av = hip.CsrDev(NROW, NCOL, rp, ci, np.ones(nnz))
    Q0 = torch.zeros((NROW, 1), dtype=_tdt(dtype), device=gpu)
    Kz = torch.zeros((NCOL, 1), dtype=_tdt(dtype), device=gpu)
    H = 3 if dv <= 64 * G2.W[dtype] else 1
    XTn, XSn, an, dOn = G2.exact_operands(dtype, H, dv, 90 + H, nrow=NROW, ncol=NCOL)
    XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
    for (A, At), v in (((A0, At0), None), ((A1, At1), val)):
        got = _g2(A, At, gpu, XT, XS, a, dO, H, 0.25, bias=v is not None)
        for h in range(H):
            s = G2.scores_dtype(rp, ci, XTn, XSn, an, 0.25, h, v)[0]
            exact = G2.scores_exact(rp, ci, XTn, XSn, an, 0.25, h, v)[0]
            assert np.array_equal(s.astype(np.longdouble), exact), "every step of the score is exact on this data"
            Av.update_values(s.astype(np.float64))
            sv = slice(h * dv, (h + 1) * dv)
            lse, p, ds = _nan(gpu, XT, NROW), _nan(gpu, XT, nnz), _nan(gpu, XT, nnz)
            O = Av.attention(Q0, Kz, XS[:, sv], scale=1.0, bias=True, lse=lse, p_out=p)
            _, delta = Av.attention_bwd_q(Q0, Kz, XS[:, sv], O, dO[:, sv], lse, scale=1.0, bias=True, ds_out=ds)
            torch.cuda.synchronize()
            mine = dict(O=got["O"][:, sv], lse=got["lse"][:, h], p=got["p"][:, h], delta=got["delta"][:, h], ds=got["ds"][:, h])
            _same(mine, dict(O=O, lse=lse, p=p, delta=delta, ds=ds), (dtype, "H = %d, dv = %d, head %d, bias %s" % (H, dv, h, v is not None)))
        assert _finite(got)
    for h in (A0, At0, A1, At1, Av):
        h.free()


# ---- b. the bound -----------------------------------------------------------------------------------------------------

def _bound_cases(dtype, dv):
    return [c for c in G2.chunk_bound_cases() if c[0] == dtype and c[2] == dv]


@pytest.mark.parametrize("dtype,dv", _by_width(G2.chunk_widths))
def test_inside_the_bound(crp, gpu, dtype, dv):
    """every output of gatv2_ref.chunk_bound_cases against the np.longdouble reference, at two scales of the scores"""
    rp, ci = G.chunk_matrix()
    A, At = _handles(rp, ci, NROW, NCOL)
    cases = _bound_cases(dtype, dv)
    assert cases
    for _, H, _, spread in cases:
        _, _, XT, XS, a, dO, ref = G2.chunk_case(dtype, H, dv, spread)
        XT, XS, a, dO = _dev(gpu, XT, XS, a, dO)
        got = _g2(A, At, gpu, XT, XS, a, dO, H, G2.SLOPE)
        assert set(got) == set(KEYS)
        _ratios(got, ref, (dtype, "H = %d, dv = %d, spread %g" % (H, dv, spread)))
    A.free()
    At.free()


# ---- c. dropout -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dv", _by_width(G2.chunk_widths))
def test_dropout_inside_the_bound(crp, gpu, dtype, dv):
    """the same cases under (DROP, SEED) against dropout_ref.gatv2_reference"""
    rp, ci = G.chunk_matrix()
    A, At = _handles(rp, ci, NROW, NCOL)
    cases = _bound_cases(dtype, dv)
    assert cases
    for _, H, _, spread in cases:
        _, _, XT, XS, a, dO, ref = D.gatv2_chunk_case(dtype, H, dv, spread)
        XT, XS, a, dO = _dev(gpu, XT, XS, a, dO)
        got = _g2_drop(A, At, gpu, XT, XS, a, dO, H, G2.SLOPE, D.DROP, D.SEED)
        _ratios_drop(got, ref, (dtype, "H = %d, dv = %d, spread %g, dropout %g" % (H, dv, spread, D.DROP)))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype,dv", _by_width(G2.chunk_widths))
def test_dropout_zero_is_the_existing_call(crp, gpu, dtype, dv):
    rp, ci = G.chunk_matrix()
    val = np.random.default_rng(8).standard_normal(ci.size)
    A, At = _handles(rp, ci, NROW, NCOL, val)
    for H in (1, 3):
        XT, XS, a, dO = _dev(gpu, *G2.operands(dtype, H, dv, 2.0, 40 + H, nrow=NROW, ncol=NCOL))
        want = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, bias=True)
        got = _g2_drop(A, At, gpu, XT, XS, a, dO, H, 0.2, 0.0, D.SEED, bias=True)
        assert set(got) == set(want)
        _same(got, want, (dtype, H, dv, "dropout = 0"))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropped_entries_with_identity_sources_and_identity_gradient(crp, gpu, dtype):
    """XS = I (dv = the number of columns; it feeds the score too, identically in both runs): O_drop == where(k, fl(O_plain rs), +0);
    with a = 0 (accZ = 0) and dO rows as unit vectors (dv = the number of rows) dXS_drop == where(k, fl(dXS_plain rs), +0) -- bit
    for bit against the plain calls, entry for entry, so every keep bit of every chunk of every row and of every column of A is
    held, on both sides; lse and p_out are the plain call's (test_gpu_gatv2_dropout.py)"""
    dt = np.dtype(dtype)
    rp, ci = G.chunk_matrix()
    A, At = _handles(rp, ci, NROW, NCOL)
    for H in (1, 3):
        k = {drop: D.mask_csr(rp, ci, H, drop, D.SEED) for drop in (D.PIN_DROP, D.DROP)}
        # the forward
        XT, _, a, _ = G2.operands(dtype, H, NCOL, 2.0, 33, nrow=NROW, ncol=NCOL)
        XT, XS, a = _dev(gpu, XT, _identity_heads(NCOL, H, dt), a)
        want = _g2(A, None, gpu, XT, XS, a, None, H, 0.2, backward=False)
        On = want["O"].cpu().numpy()
        for drop in k:
            rs = D.rs_of(drop, dt)
            got = _g2_drop(A, None, gpu, XT, XS, a, None, H, 0.2, drop, D.SEED, backward=False)
            _same(got, want, (dtype, H, drop, "lse and p_out"), keys=("lse", "p"))
            mine = got["O"].cpu().numpy()
            for h in range(H):
                sv = slice(h * NCOL, (h + 1) * NCOL)
                K = D.dense_mask(rp, ci, NCOL, k[drop][:, h])
                exp = np.where(K, (On[:, sv] * rs).astype(dt), dt.type(0))
                assert np.array_equal(mine[:, sv], exp) and not np.signbit(mine[:, sv][~K]).any(), (dtype, H, drop, h, "O")
        # the column side
        XT, XS, a, _ = G2.operands(dtype, H, NROW, 2.0, 34, nrow=NROW, ncol=NCOL)
        XT, XS, a, dO = _dev(gpu, XT, XS, np.zeros_like(a), _identity_heads(NROW, H, dt))
        want = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2)["dXS"].cpu().numpy()
        for drop in k:
            rs = D.rs_of(drop, dt)
            got = _g2_drop(A, At, gpu, XT, XS, a, dO, H, 0.2, drop, D.SEED)["dXS"].cpu().numpy()
            for h in range(H):
                sv = slice(h * NROW, (h + 1) * NROW)
                Kt = D.dense_mask(rp, ci, NCOL, k[drop][:, h]).T
                exp = np.where(Kt, (want[:, sv] * rs).astype(dt), dt.type(0))
                assert np.array_equal(got[:, sv], exp), (dtype, H, drop, h, "dXS")
    A.free()
    At.free()


# ---- d. invariances that depend on length -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dv", _by_width(_invariance_widths))
def test_invariance(crp, gpu, dtype, dv):
    """two sources against one, forward and row side; head h of an H = 3 call against the one-head call on its column views; an odd
    leading dimension with an offset pointer against the aligned call, without and with dropout -- all bit for bit"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.chunk_matrix()
    nnz = ci.size
    val = np.random.default_rng(3).standard_normal(nnz)
    A, At = _handles(rp, ci, NROW, NCOL, val)
    H = 3
    XTn, XSn, an, dOn = G2.operands(dtype, H, dv, 2.0, 31, nrow=NROW, ncol=NCOL)
    XT, XS, a, dO = _dev(gpu, XTn, XSn, an, dOn)
    want = _g2(A, At, gpu, XT, XS, a, dO, H, 0.2, bias=True)
    # two sources
    A2 = hip.CsrDev(NROW, K0, rp, G.two_source_codes(ci, K0), val)
    got = _g2(A2, None, gpu, XT, XS[:K0], a, dO, H, 0.2, bias=True, XS1=XS[K0:])
    _same(got, want, (dtype, dv, "two sources"))
    A2.free()
    # head h of the H-head call against the one-head call on head h's column views
    for h in range(H):
        sv = slice(h * dv, (h + 1) * dv)
        one = _g2(A, At, gpu, XT[:, sv], XS[:, sv], a[h].clone(), dO[:, sv], 1, 0.2, bias=True)
        mine = {k: (want[k][sv] if k == "da" else want[k][:, sv] if k in ("O", "dXT", "da_part", "dXS") else want[k][:, h:h + 1])
                for k in KEYS}
        _same(one, mine, (dtype, dv, "head %d against the one-head call" % h))
    # an odd leading dimension and an offset pointer: the element path
    for drop in (0.0, D.PIN_DROP):
        kw = dict(slope=0.2, bias=True, heads=H, **(dict(dropout=drop, seed=D.SEED) if drop else {}))
        base = _g2_drop(A, At, gpu, XT, XS, a, dO, H, 0.2, drop, D.SEED, bias=True) if drop else want
        ld_extra, off = 3, 1
        sXT, sXS, sdO = (_strided(gpu, t, t.shape[1] + ld_extra, off) for t in (XTn, XSn, dOn))
        sa = a if drop else _strided(gpu, an.reshape(1, -1), H * dv, off)[0]        # (as in the tests of the 40 x 80 pattern)
        mk = lambda r: _strided(gpu, np.zeros((r, H * dv), dtype), H * dv + ld_extra, off)
        O, dXT, da_part, dXS = mk(NROW), mk(NROW), mk(NROW), mk(NCOL)
        lse, p, ds, delta = _nan(gpu, XT, NROW, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, nnz, H), _nan(gpu, XT, NROW, H)
        A.gatv2_attention(sXT, sXS, sa, out=O, lse=lse, p_out=p, **kw)
        A.gatv2_attention_bwd_row(sXT, sXS, sa, O, sdO, lse, dXT=dXT, da_part=da_part, delta=delta, ds_out=ds, **kw)
        At.gatv2_attention_bwd_col(sXS, sXT, sa, sdO, lse, delta, dXS=dXS, **kw)
        da = hip.col_sum(da_part)
        torch.cuda.synchronize()
        got = dict(O=O.contiguous(), lse=lse, p=p, delta=delta, ds=ds, dXT=dXT.contiguous(), da_part=da_part.contiguous(),
                   dXS=dXS.contiguous(), da=da)
        _same(got, base, (dtype, dv, "ld + %d, offset %d, dropout %g" % (ld_extra, off, drop)))
    A.free()
    At.free()
