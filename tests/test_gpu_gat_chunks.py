"""GPU: the fused GAT attention, its two-handle backward and their dropout variants on gat_ref.chunk_matrix() -- rows of 0, 1, 7, 8,
9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129 and 200 entries, the long ones in shuffled column order, a hub column of 277 entries
and columns of exactly 0, 1, 8, 9, 63, 64 and 65: every edge of a chunk of LPR = 8, 16, 32 and 64 entries and up to five chunks of
64, on the row side and on the column side -- at gat_ref.chunk_widths(): both sides of every threshold of the dispatch tables, the
cap (P = 4, full), the forward's P = 8 in one V block, and element-path widths inside the 32- and the 64-lane range.

Every output of the forward, the row side and the column side is held
  a. bit for bit against kernels that are pinned on such patterns themselves (test_gpu_attention*.py): the slope-1 two-column trick
     at every width, the scores-as-values pin for the other slopes at one width per instance;
  b. inside the bound of DESIGN.md 5o against the np.longdouble reference;
  c. under dropout: inside the bound of 5q at (DROP, SEED); dropout = 0 against the plain call; the mask of both handles against
     numpy's Philox; and, with V = I and with dO = I, the dropped O and dV against the plain call's, entry for entry -- which holds
     every keep bit of every chunk of the long rows and of the hub column;
  d. against itself where the answer must not depend on the layout: two sources against one, head h of three against the one-head
     call, an odd leading dimension with an offset pointer (the element path) against the aligned call (the 16-byte path)."""
import numpy as np
import pytest

import attention_bwd_ref as B
import dropout_ref as D
import gat_ref as G
from test_gpu_attention import _strided
from test_gpu_gat import KEYS, SLOPES, _dev, _gat, _handles, _nan, _pin_by_values, _ratios, _same
from test_gpu_gat_dropout import _gat as _gat_drop
from test_gpu_gat_dropout import _ratios as _ratios_drop

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
NROW, NCOL, K0 = G.CHUNK_NROW, G.CHUNK_NCOL, G.CHUNK_K0


def _cap(dtype):
    return B.CAP[np.dtype(dtype)]


def _by_width(widths):
    """(dtype, dv) pairs as pytest parameters"""
    return [pytest.param(dtype, dv, id="%s-%d" % (dtype, dv)) for dtype in DTYPES for dv in widths(dtype)]


def _pin_widths(dtype):
    """every width of the chunk pattern and the widths of the 40 x 80 pattern, one or more per instance"""
    return tuple(sorted(set(G.chunk_widths(dtype, "gat_fwd")) | set(G.widths(dtype))))


def _value_pin_widths(dtype):
    """one width per (LPR, P) of the backward's table, 16-byte and element path in turn"""
    w = G.W[dtype]
    out = (5, 16 * w, 17 * w + 1, 64 * w, 64 * w + 1, 256 * w)
    assert [G.instance_of("gat_bwd", dtype, dv) for dv in out] == [inst for _, inst in G.INSTANCES]
    return out


def _invariance_widths(dtype):
    """a 16-byte and an element-path width in the 32-lane range and in the P = 4 range"""
    w = G.W[dtype]
    out = (32 * w, 17 * w + 1, 256 * w, 128 * w + 1)
    assert [G.instance_of("gat_bwd", dtype, dv) for dv in out] == [(32, 1), (32, 1), (64, 4), (64, 4)]
    return out


def _identity_heads(n, H, dt):
    return np.tile(np.eye(n, dtype=dt), (1, H))


# ---- a. bit pins ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dv", _by_width(_pin_widths))
def test_slope_one_equals_the_attention_with_two_columns(crp, gpu, dtype, dv):
    """the fused attention with dk = 2 on Q_h = [el_h, 1], K_h = [1, er_h], scale = 1 (test_gpu_gat.py); past the backward's cap the
    forward alone"""
    import torch
    rp, ci = G.chunk_matrix()
    val = np.random.default_rng(8).standard_normal(ci.size)
    A, At = _handles(rp, ci, NROW, NCOL, val)
    backward = dv <= _cap(dtype)
    for H in (1, 3):
        el, er, V, dO = _dev(gpu, *G.operands(dtype, H, dv, 2.0, 50 + H, nrow=NROW, ncol=NCOL))
        Q = torch.ones((NROW, 2 * H), dtype=V.dtype, device=gpu)
        K = torch.ones((NCOL, 2 * H), dtype=V.dtype, device=gpu)
        Q[:, 0::2], K[:, 1::2] = el, er
        flat = (lambda t: t.view(-1)) if H == 1 else (lambda t: t)
        for bias in (False, True):
            lse, p, ds = _nan(gpu, V, NROW, H), _nan(gpu, V, ci.size, H), _nan(gpu, V, ci.size, H)
            O = A.attention(Q, K, V, scale=1.0, bias=bias, lse=flat(lse), p_out=flat(p), heads=H)
            want = dict(O=O, lse=lse, p=p)
            if backward:
                dQ, delta = A.attention_bwd_q(Q, K, V, O, dO, flat(lse), scale=1.0, bias=bias, ds_out=flat(ds), heads=H)
                dK, dV = At.attention_bwd_kv(K, V, Q, dO, flat(lse), flat(delta), scale=1.0, bias=bias, heads=H)
                want.update(delta=delta.view(NROW, H), ds=ds, d_el=dQ[:, 0::2].contiguous(), d_er=dK[:, 1::2].contiguous(), dV=dV)
            torch.cuda.synchronize()
            got = _gat(A, At, gpu, el, er, V, dO, H, 1.0, bias=bias, backward=backward)
            assert set(got) == set(want)
            if backward:
                got["d_el"], got["d_er"] = got["d_el"].contiguous(), got["d_er"].contiguous()
            _same(got, want, (dtype, H, dv, "bias" if bias else "no bias"))
            assert all(bool(got[k].isfinite().all()) for k in got if k != "lse")
    A.free()
    At.free()


@pytest.mark.parametrize("dtype,dv", _by_width(_value_pin_widths))
def test_any_slope_equals_the_attention_on_scores_as_values(crp, gpu, dtype, dv):
    """the single-head attention with Q = 0 and bias = 1 on a handle whose values are lrelu(fl(el + er)), formed by numpy in the
    dtype; d_el and d_er are numpy's sequential sums of that run's ds_out times g (test_gpu_gat.py) -- the hub column's 277 terms"""
    rp, ci = G.chunk_matrix()
    A, At = _handles(rp, ci, NROW, NCOL)
    Av, Atv = _handles(rp, ci, NROW, NCOL)
    H = 3 if dv <= 64 * G.W[dtype] else 1
    el, er, V, dO = _dev(gpu, *G.operands(dtype, H, dv, 3.0, 70 + H, nrow=NROW, ncol=NCOL))
    for slope in SLOPES:
        got = _pin_by_values(gpu, dtype, rp, ci, NROW, NCOL, A, At, Av, Atv, el, er, V, dO, H, slope)
        assert all(bool(got[k].isfinite().all()) for k in KEYS if k != "lse")
    for h in (A, At, Av, Atv):
        h.free()


# ---- b. the bound -----------------------------------------------------------------------------------------------------

def _bound_cases(dtype, dv):
    return [c for c in G.chunk_bound_cases() if c[0] == dtype and c[2] == dv]


@pytest.mark.parametrize("dtype,dv", _by_width(lambda dtype: G.chunk_widths(dtype, "gat_fwd")))
def test_inside_the_bound(crp, gpu, dtype, dv):
    """every output of gat_ref.chunk_bound_cases against the np.longdouble reference, at two scales of the scores"""
    rp, ci = G.chunk_matrix()
    A, At = _handles(rp, ci, NROW, NCOL)
    cases = _bound_cases(dtype, dv)
    assert cases
    for _, H, _, spread, backward in cases:
        _, _, el, er, V, dO, ref = G.chunk_case(dtype, H, dv, spread, backward)
        el, er, V = _dev(gpu, el, er, V)
        dO = _dev(gpu, dO)[0] if backward else None
        got = _gat(A, At, gpu, el, er, V, dO, H, G.SLOPE, backward=backward)
        assert set(got) == set(G.FWD_KEYS + (G.BWD_KEYS if backward else ()))
        _ratios(got, ref, (dtype, "H = %d, dv = %d, spread %g" % (H, dv, spread)))
    A.free()
    At.free()


# ---- c. dropout -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dv", _by_width(lambda dtype: G.chunk_widths(dtype, "gat_fwd")))
def test_dropout_inside_the_bound(crp, gpu, dtype, dv):
    """the same cases under (DROP, SEED) against dropout_ref.gat_reference: a keep bit taken from the wrong chunk, or
    lane, of a long row or of the hub column moves an output by a whole term"""
    rp, ci = G.chunk_matrix()
    A, At = _handles(rp, ci, NROW, NCOL)
    cases = _bound_cases(dtype, dv)
    assert cases
    for _, H, _, spread, backward in cases:
        _, _, el, er, V, dO, ref = D.gat_chunk_case(dtype, H, dv, spread, backward)
        el, er, V = _dev(gpu, el, er, V)
        dO = _dev(gpu, dO)[0] if backward else None
        got = _gat_drop(A, At, gpu, el, er, V, dO, H, G.SLOPE, D.DROP, D.SEED, backward=backward)
        _ratios_drop(got, ref, (dtype, "H = %d, dv = %d, spread %g, dropout %g" % (H, dv, spread, D.DROP)))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype,dv", _by_width(lambda dtype: G.chunk_widths(dtype, "gat_fwd")))
def test_dropout_zero_is_the_existing_call(crp, gpu, dtype, dv):
    rp, ci = G.chunk_matrix()
    val = np.random.default_rng(8).standard_normal(ci.size)
    A, At = _handles(rp, ci, NROW, NCOL, val)
    backward = dv <= _cap(dtype)
    for H in (1, 3):
        el, er, V, dO = _dev(gpu, *G.operands(dtype, H, dv, 2.0, 40 + H, nrow=NROW, ncol=NCOL))
        want = _gat(A, At, gpu, el, er, V, dO, H, 0.2, bias=True, backward=backward)
        got = _gat_drop(A, At, gpu, el, er, V, dO, H, 0.2, 0.0, D.SEED, bias=True, backward=backward)
        assert set(got) == set(want)
        _same(got, want, (dtype, H, dv, "dropout = 0"))
    A.free()
    At.free()


def test_dropout_mask_is_numpys(crp, gpu):
    """over A, over A^T -- the hub column's five chunks of 64 -- and over the two-source codes"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = G.chunk_matrix()
    nnz = ci.size
    A, At = _handles(rp, ci, NROW, NCOL)
    tmap = B.transpose(rp, ci, NCOL)[2]
    for H in (1, 3):
        for drop, seed in ((D.DROP, D.SEED), (D.PIN_DROP, 7)):
            want = D.mask_csr(rp, ci, H, drop, seed)
            m, mt = A.dropout_mask(H, drop, seed), At.dropout_mask(H, drop, seed)
            torch.cuda.synchronize()
            assert tuple(m.shape) == (nnz, H) and tuple(mt.shape) == (nnz, H)
            assert np.array_equal(m.cpu().numpy(), want.astype(np.uint8)), (H, drop, "over A")
            assert np.array_equal(mt.cpu().numpy(), want[tmap].astype(np.uint8)), (H, drop, "over A^T: the same bits, transposed")
    codes = G.two_source_codes(ci, K0)
    A2 = hip.CsrDev(NROW, K0, rp, codes, np.ones(nnz))
    got = A2.dropout_mask(3, D.DROP, D.SEED).cpu().numpy()
    assert np.array_equal(got, D.mask_csr(rp, codes, 3, D.DROP, D.SEED).astype(np.uint8))
    for h in (A, At, A2):
        h.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropped_entries_with_identity_values_and_identity_gradient(crp, gpu, dtype):
    """V = I (dv = the number of columns): every column of O holds one entry's term, so O_drop == where(k, fl(O_plain rs), +0); with
    dO rows as unit vectors (dv = the number of rows) dV_drop == where(k, fl(dV_plain rs), +0) -- bit for bit against the plain
    calls, entry for entry, so every keep bit of every chunk of every row and of every column of A is held, on both sides; lse and
    p_out are the plain call's (test_gpu_gat_dropout.py)"""
    dt = np.dtype(dtype)
    rp, ci = G.chunk_matrix()
    A, At = _handles(rp, ci, NROW, NCOL)
    for H in (1, 3):
        k = {drop: D.mask_csr(rp, ci, H, drop, D.SEED) for drop in (D.PIN_DROP, D.DROP)}
        # the forward
        el, er, _, _ = G.operands(dtype, H, 1, 2.0, 33, nrow=NROW, ncol=NCOL)
        el, er, V = _dev(gpu, el, er, _identity_heads(NCOL, H, dt))
        want = _gat(A, None, gpu, el, er, V, None, H, 0.2, backward=False)
        On = want["O"].cpu().numpy()
        for drop in k:
            rs = D.rs_of(drop, dt)
            got = _gat_drop(A, None, gpu, el, er, V, None, H, 0.2, drop, D.SEED, backward=False)
            _same(got, want, (dtype, H, drop, "lse and p_out"), keys=("lse", "p"))
            mine = got["O"].cpu().numpy()
            for h in range(H):
                sv = slice(h * NCOL, (h + 1) * NCOL)
                K = D.dense_mask(rp, ci, NCOL, k[drop][:, h])
                exp = np.where(K, (On[:, sv] * rs).astype(dt), dt.type(0))
                assert np.array_equal(mine[:, sv], exp) and not np.signbit(mine[:, sv][~K]).any(), (dtype, H, drop, h, "O")
        # the column side
        el, er, V, _ = G.operands(dtype, H, NROW, 2.0, 34, nrow=NROW, ncol=NCOL)
        el, er, V, dO = _dev(gpu, el, er, V, _identity_heads(NROW, H, dt))
        want = _gat(A, At, gpu, el, er, V, dO, H, 0.2)["dV"].cpu().numpy()
        for drop in k:
            rs = D.rs_of(drop, dt)
            got = _gat_drop(A, At, gpu, el, er, V, dO, H, 0.2, drop, D.SEED)["dV"].cpu().numpy()
            for h in range(H):
                sv = slice(h * NROW, (h + 1) * NROW)
                Kt = D.dense_mask(rp, ci, NCOL, k[drop][:, h]).T
                exp = np.where(Kt, (want[:, sv] * rs).astype(dt), dt.type(0))
                assert np.array_equal(got[:, sv], exp) and not np.signbit(got[:, sv][~Kt]).any(), (dtype, H, drop, h, "dV")
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
    eln, ern, Vn, dOn = G.operands(dtype, H, dv, 2.0, 31, nrow=NROW, ncol=NCOL)
    el, er, V, dO = _dev(gpu, eln, ern, Vn, dOn)
    want = _gat(A, At, gpu, el, er, V, dO, H, 0.2, bias=True)
    # two sources
    A2 = hip.CsrDev(NROW, K0, rp, G.two_source_codes(ci, K0), val)
    got = _gat(A2, None, gpu, el, er[:K0], V[:K0], dO, H, 0.2, bias=True, er1=er[K0:], V1=V[K0:])
    _same(got, want, (dtype, dv, "two sources"))
    A2.free()
    # head h of the H-head call against the one-head call on head h's column views
    for h in range(H):
        sv = slice(h * dv, (h + 1) * dv)
        one = _gat(A, At, gpu, el[:, h:h + 1], er[:, h:h + 1], V[:, sv], dO[:, sv], 1, 0.2, bias=True)
        mine = {k: (want[k][:, sv] if k in ("O", "dV") else want[k][:, h:h + 1]) for k in KEYS}
        _same(one, mine, (dtype, dv, "head %d against the one-head call" % h))
    # an odd leading dimension and an offset pointer: the element path
    for drop in (0.0, D.PIN_DROP):
        kw = dict(slope=0.2, bias=True, heads=H, **(dict(dropout=drop, seed=D.SEED) if drop else {}))
        base = _gat_drop(A, At, gpu, el, er, V, dO, H, 0.2, drop, D.SEED, bias=True) if drop else want
        ld_extra, off = 3, 1
        sel, ser, sV, sdO = (_strided(gpu, t, t.shape[1] + ld_extra, off) for t in (eln, ern, Vn, dOn))
        O = _strided(gpu, np.zeros((NROW, H * dv), dtype), H * dv + ld_extra, off)
        dV = _strided(gpu, np.zeros((NCOL, H * dv), dtype), H * dv + ld_extra, off)
        d_el = _strided(gpu, np.zeros((NROW, H), dtype), H + ld_extra, off)
        d_er = _strided(gpu, np.zeros((NCOL, H), dtype), H + ld_extra, off)
        lse, p, ds, delta = _nan(gpu, V, NROW, H), _nan(gpu, V, nnz, H), _nan(gpu, V, nnz, H), _nan(gpu, V, NROW, H)
        A.gat_attention(sel, ser, sV, out=O, lse=lse, p_out=p, **kw)
        A.gat_attention_bwd_row(sel, ser, sV, O, sdO, lse, d_el=d_el, delta=delta, ds_out=ds, **kw)
        At.gat_attention_bwd_col(ser, sV, sel, sdO, lse, delta, d_er=d_er, dV=dV, **kw)
        torch.cuda.synchronize()
        got = dict(O=O.contiguous(), lse=lse, p=p, delta=delta, ds=ds, d_el=d_el.contiguous(), d_er=d_er.contiguous(), dV=dV.contiguous())
        _same(got, base, (dtype, dv, "ld + %d, offset %d, dropout %g" % (ld_extra, off, drop)))
    A.free()
    At.free()
