"""GPU: multi-head batching of the fused sparse attention and its backward (crp_attention_mh_csr_*,
crp_attention_bwd_q_mh_csr_*, crp_attention_bwd_kv_mh_csr_*, the ``heads`` keyword of the wrappers and of hip.sparse_attention).

The oracle is the bit contract of DESIGN.md 5n: head h of every output of a multi-head call equals, bit for bit, the existing
single-head call with nk = dk, nv = dv on the column views of head h (the same leading dimensions).  Every comparison below is
torch.equal; one case per dtype is also held against attention_ref.reference per head, inside 5j's bound, as an anchor that does
not go through the single-head kernels.  Pattern: attention_ref.matrix() -- 256 rows of 0, 1, 7, 8, 9, 63, 64, 65, 200, 5000, ...
entries -- and attention_ref.steep_case's rows with the bias as values, masked entries and one all-masked row."""
import functools

import numpy as np
import pytest

import attention_bwd_ref as B
import attention_ref as R
from test_gpu_attention import SENT, _check, _strided, _tdt

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
KEYS = ("O", "lse", "p", "dQ", "delta", "ds", "dK", "dV")
W = {"float64": 2, "float32": 4}


def _operands(gpu, dtype, nrow, ncol, H, dk, dv, seed, ld_extra=0, off=0):
    """Q, K, V, dO with H heads side by side (standard normal, made once on the host) and the scale 1 / sqrt(dk); ld_extra, off: an
    odd leading dimension and a base pointer `off` elements into the allocation"""
    import torch
    g = torch.Generator().manual_seed(seed)
    mk = lambda r, c: torch.randn((r, c), generator=g, dtype=torch.float64).to(_tdt(dtype))
    ops = [mk(nrow, H * dk), mk(ncol, H * dk), mk(ncol, H * dv), mk(nrow, H * dv)]
    if ld_extra or off:
        ops = [_strided(gpu, t.numpy(), t.shape[1] + ld_extra, off) for t in ops]
    else:
        ops = [t.to(gpu) for t in ops]
    return ops + [float(np.dtype(dtype).type(1.0 / np.sqrt(dk)))]


def _nan(gpu, like, *shape):
    import torch
    return torch.full(shape, float("nan"), dtype=like.dtype, device=gpu)


def _multi(A, At, gpu, Q, K, V, dO, H, scale, bias=False, K1=None, V1=None, inplace=False):
    """one multi-head forward, bwd_q and (At given) bwd_kv -> dict of device tensors; inplace: the column side with dK is K, dV is V"""
    import torch
    nrow, nnz = Q.shape[0], A.nnz
    lse, p, ds = _nan(gpu, Q, nrow, H), _nan(gpu, Q, nnz, H), _nan(gpu, Q, nnz, H)
    O = A.attention(Q, K, V, K1=K1, V1=V1, scale=scale, bias=bias, lse=lse, p_out=p, heads=H)
    dQ, delta = A.attention_bwd_q(Q, K, V, O, dO, lse, K1=K1, V1=V1, scale=scale, bias=bias, ds_out=ds, heads=H)
    out = dict(O=O, lse=lse, p=p, dQ=dQ, delta=delta, ds=ds)
    if At is not None:
        if inplace:
            Kc, Vc = K.clone(), V.clone()
            dK, dV = At.attention_bwd_kv(Kc, Vc, Q, dO, lse, delta, scale=scale, bias=bias, dK=Kc, dV=Vc, heads=H)
            assert dK is Kc and dV is Vc
        else:
            dK, dV = At.attention_bwd_kv(K, V, Q, dO, lse, delta, scale=scale, bias=bias, heads=H)
        out.update(dK=dK, dV=dV)
    torch.cuda.synchronize()
    return out


def _single(A, At, gpu, Q, K, V, dO, H, scale, bias=False):
    """the oracle: H single-head calls of each kind on the column views of head h, assembled in the multi-head layout"""
    import torch
    nrow, ncol, nnz = Q.shape[0], K.shape[0], A.nnz
    dk, dv = Q.shape[1] // H, V.shape[1] // H
    O, dQ = _nan(gpu, Q, nrow, H * dv), _nan(gpu, Q, nrow, H * dk)
    dK, dV = _nan(gpu, Q, ncol, H * dk), _nan(gpu, Q, ncol, H * dv)
    lse, delta = _nan(gpu, Q, H, nrow), _nan(gpu, Q, H, nrow)
    p, ds = _nan(gpu, Q, H, max(nnz, 1))[:, :nnz].contiguous(), _nan(gpu, Q, H, max(nnz, 1))[:, :nnz].contiguous()
    for h in range(H):
        sk, sv = slice(h * dk, (h + 1) * dk), slice(h * dv, (h + 1) * dv)
        A.attention(Q[:, sk], K[:, sk], V[:, sv], scale=scale, bias=bias, out=O[:, sv], lse=lse[h], p_out=p[h])
        A.attention_bwd_q(Q[:, sk], K[:, sk], V[:, sv], O[:, sv], dO[:, sv], lse[h], scale=scale, bias=bias, dQ=dQ[:, sk], delta=delta[h],
                          ds_out=ds[h])
        if At is not None:
            At.attention_bwd_kv(K[:, sk], V[:, sv], Q[:, sk], dO[:, sv], lse[h], delta[h], scale=scale, bias=bias, dK=dK[:, sk], dV=dV[:, sv])
    torch.cuda.synchronize()
    out = dict(O=O, lse=lse.t().contiguous(), p=p.t().contiguous(), dQ=dQ, delta=delta.t().contiguous(), ds=ds.t().contiguous())
    if At is not None:
        out.update(dK=dK, dV=dV)
    return out


def _same(got, want, what):
    import torch
    for k in KEYS:
        if k in got and k in want:
            assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
            assert torch.equal(got[k], want[k]), (what, k, "differs from the single-head calls on the column views")


def _handles(rp, ci, nrow, ncol, val=None):
    from crp_spmm_amd import hip
    val = np.ones(ci.size) if val is None else val
    return hip.CsrDev(nrow, ncol, rp, ci, val), hip.CsrDev.from_transpose(nrow, ncol, rp, ci, val)


def _matrix(nrow=R.NROW):
    """attention_ref.matrix(), or its first nrow rows"""
    rp, ci = R.matrix()
    return rp[:nrow + 1], ci[:int(rp[nrow])]


# (dk, dv) per lane group L = 8, 16, 32, 64 and the wave instance that keeps two pieces of Q (PK = 2), per dtype
INSTANCES = {"float64": {8: (8, 8), 16: (24, 20), 32: (8, 40), 64: (66, 64), "PK2": (130, 4)},
             "float32": {8: (8, 8), 16: (48, 40), 32: (16, 80), 64: (132, 128), "PK2": (260, 4)}}


def test_the_instances_are_the_ones_meant():
    for dtype, table in INSTANCES.items():
        for key, (dk, dv) in table.items():
            lpr, pk, _ = R.instance_of(dk, dv, dtype)
            assert (lpr, pk) == ((64, 2) if key == "PK2" else (key, 1)), (dtype, key, lpr, pk)


@pytest.mark.parametrize("dtype", DTYPES)
def test_heads_against_the_group_of_eight_lanes(crp, gpu, dtype):
    """L = 8: a wave holds 8 units.  H = 2, 3, 5, 8, 16: below, coprime to, equal to and above 64 / L.  On all 256 rows (every
    block full) and on the first 255 (the last block partial; H = 2, 3, 5 leave the last wave partial too)"""
    dk, dv = INSTANCES[dtype][8]
    for nrow in (R.NROW, R.NROW - 1):
        rp, ci = _matrix(nrow)
        A, At = _handles(rp, ci, nrow, R.NCOL)
        for H in (2, 3, 5, 8, 16):
            Q, K, V, dO, scale = _operands(gpu, dtype, nrow, R.NCOL, H, dk, dv, 10 * H + nrow)
            got = _multi(A, At, gpu, Q, K, V, dO, H, scale)
            _same(got, _single(A, At, gpu, Q, K, V, dO, H, scale), (dtype, nrow, H))
            empty = np.flatnonzero(np.diff(rp) == 0)
            assert empty.size and bool((got["lse"][empty] == -np.inf).all()), "an empty row: lse = -inf for every head"
            assert bool((got["O"][empty] == 0).all()) and not bool(got["O"][empty].signbit().any())
            assert all(bool(got[k].isfinite().all()) for k in KEYS if k != "lse")
        A.free()
        At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_lane_group(crp, gpu, dtype):
    """one instance per L = 16, 32, 64 and the PK = 2 wave instance, with H = 3 (and H = 2 for the widest); the column side in
    place over K and V (dK is K, dV is V) and out of place"""
    rp, ci = _matrix()
    A, At = _handles(rp, ci, R.NROW, R.NCOL)
    for key, H in ((16, 3), (32, 3), (64, 2), ("PK2", 3)):
        dk, dv = INSTANCES[dtype][key]
        Q, K, V, dO, scale = _operands(gpu, dtype, R.NROW, R.NCOL, H, dk, dv, 7)
        want = _single(A, At, gpu, Q, K, V, dO, H, scale)
        _same(_multi(A, At, gpu, Q, K, V, dO, H, scale), want, (dtype, key, H))
        _same(_multi(A, At, gpu, Q, K, V, dO, H, scale, inplace=True), want, (dtype, key, H, "dK is K, dV is V"))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_slices_leading_dimensions_and_pointers(crp, gpu, dtype):
    """(dk, dv) = (33, 33) and (3, 5) with H > 1: under an aligned base the slices of heads 1, 2, ... are not on 16-byte
    boundaries, so the element path has to serve them; an aligned instance with an odd leading dimension and with a base pointer one
    element into its allocation (outputs included)"""
    import torch
    rp, ci = _matrix()
    A, At = _handles(rp, ci, R.NROW, R.NCOL)
    for dk, dv, H in ((33, 33, 3), (3, 5, 4)):
        Q, K, V, dO, scale = _operands(gpu, dtype, R.NROW, R.NCOL, H, dk, dv, 3)
        assert all(t.data_ptr() % 16 == 0 for t in (Q, K, V, dO))
        _same(_multi(A, At, gpu, Q, K, V, dO, H, scale), _single(A, At, gpu, Q, K, V, dO, H, scale), (dtype, dk, dv, H))
    dk, dv = INSTANCES[dtype][16]
    H = 3
    Q, K, V, dO, scale = _operands(gpu, dtype, R.NROW, R.NCOL, H, dk, dv, 5)
    want = _single(A, At, gpu, Q, K, V, dO, H, scale)
    for ld_extra, off in ((1, 0), (0, 1), (3, 1)):
        sQ, sK, sV, sdO = (_strided(gpu, t.cpu().numpy(), t.shape[1] + ld_extra, off) for t in (Q, K, V, dO))
        lse, p, ds, delta = _nan(gpu, Q, R.NROW, H), _nan(gpu, Q, A.nnz, H), _nan(gpu, Q, A.nnz, H), _nan(gpu, Q, R.NROW, H)
        O = _strided(gpu, np.zeros((R.NROW, H * dv), dtype), H * dv + ld_extra, off)
        dQ = _strided(gpu, np.zeros((R.NROW, H * dk), dtype), H * dk + ld_extra, off)
        dK = _strided(gpu, np.zeros((R.NCOL, H * dk), dtype), H * dk + ld_extra, off)
        dV = _strided(gpu, np.zeros((R.NCOL, H * dv), dtype), H * dv + ld_extra, off)
        A.attention(sQ, sK, sV, scale=scale, out=O, lse=lse, p_out=p, heads=H)
        A.attention_bwd_q(sQ, sK, sV, O, sdO, lse, scale=scale, dQ=dQ, delta=delta, ds_out=ds, heads=H)
        At.attention_bwd_kv(sK, sV, sQ, sdO, lse, delta, scale=scale, dK=dK, dV=dV, heads=H)
        torch.cuda.synchronize()
        got = dict(O=O.contiguous(), lse=lse, p=p, dQ=dQ.contiguous(), delta=delta, ds=ds, dK=dK.contiguous(), dV=dV.contiguous())
        _same(got, want, (dtype, "ld + %d, offset %d" % (ld_extra, off)))
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_sources_row_subsets_and_out_pos(crp, gpu, dtype):
    """K1 / V1 through negative column codes; two row-subset handles with row maps that write one set of outputs through their
    positions; out_pos as a permutation of a full handle"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = _matrix()
    nrow, nnz = R.NROW, ci.size
    rows = R.rows_of(rp)
    A, At = _handles(rp, ci, nrow, R.NCOL)
    H = 3
    dk, dv = INSTANCES[dtype][8]
    Q, K, V, dO, scale = _operands(gpu, dtype, nrow, R.NCOL, H, dk, dv, 21)
    want = _single(A, At, gpu, Q, K, V, dO, H, scale)
    # two sources
    k0 = 2000
    codes = np.where(ci < k0, ci, ~(ci - k0)).astype(np.int32)
    A2 = hip.CsrDev(nrow, k0, rp, codes, np.ones(nnz))
    _same(_multi(A2, None, gpu, Q, K[:k0], V[:k0], dO, H, scale, K1=K[k0:], V1=V[k0:]), want, (dtype, "two sources"))
    A2.free()
    # row subsets with a row map, writing through their positions
    O, dQ = _nan(gpu, Q, nrow, H * dv), _nan(gpu, Q, nrow, H * dk)
    lse, delta, p, ds = _nan(gpu, Q, nrow, H), _nan(gpu, Q, nrow, H), _nan(gpu, Q, nnz, H), _nan(gpu, Q, nnz, H)
    pick = (np.arange(nrow) % 4) % 3 == 0
    for sel in (pick, ~pick):
        r = np.flatnonzero(sel)
        keep = sel[rows]
        h = hip.CsrDev(r.size, R.NCOL, np.concatenate([[0], np.cumsum(np.diff(rp)[r])]).astype(np.int32), ci[keep], np.ones(int(keep.sum())))
        h.set_rowmap(r, nrow)
        pos = torch.from_numpy(np.flatnonzero(keep).astype(np.int32)).to(gpu)
        h.attention(Q, K, V, scale=scale, out=O, lse=lse, p_out=p, out_pos=pos, heads=H)
        h.attention_bwd_q(Q, K, V, O, dO, lse, scale=scale, dQ=dQ, delta=delta, ds_out=ds, out_pos=pos, heads=H)
        torch.cuda.synchronize()
        h.free()
    _same(dict(O=O, lse=lse, p=p, dQ=dQ, delta=delta, ds=ds), want, (dtype, "row subsets"))
    # out_pos as a permutation: nonzero q's heads land in row perm[q]
    perm = np.random.default_rng(2).permutation(nnz).astype(np.int32)
    pos = torch.from_numpy(perm).to(gpu)
    lse, p, ds = _nan(gpu, Q, nrow, H), _nan(gpu, Q, nnz, H), _nan(gpu, Q, nnz, H)
    O = A.attention(Q, K, V, scale=scale, lse=lse, p_out=p, out_pos=pos, heads=H)
    A.attention_bwd_q(Q, K, V, O, dO, lse, scale=scale, ds_out=ds, out_pos=pos, heads=H)
    torch.cuda.synchronize()
    idx = torch.from_numpy(perm.astype(np.int64)).to(gpu)
    assert torch.equal(p[idx], want["p"]) and torch.equal(ds[idx], want["ds"]), (dtype, "out_pos as a permutation")
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_masked_edges_and_an_all_masked_row(crp, gpu, dtype):
    """attention_ref.steep_case's rows -- ramps that raise the maximum in every batch, a maximum in the last partial batch, every
    second entry masked -- with the bias as the handles' values, shared by the heads, and one row masked altogether"""
    rp, ci, bias, _, _, _, scale, _ = R.steep_case(dtype)
    bias = bias.copy()
    dead = 6
    bias[rp[dead]:rp[dead + 1]] = -np.inf
    nrow, ncol = rp.size - 1, 80
    A, At = _handles(rp, ci, nrow, ncol, bias)
    for H, (dk, dv) in ((3, (24, 20)), (5, INSTANCES[dtype][8])):
        Q, K, V, dO, _ = _operands(gpu, dtype, nrow, ncol, H, dk, dv, 13)
        got = _multi(A, At, gpu, Q, K, V, dO, H, scale, bias=True)
        _same(got, _single(A, At, gpu, Q, K, V, dO, H, scale, bias=True), (dtype, H, dk, dv))
        masked = np.flatnonzero(~np.isfinite(bias))
        assert bool((got["p"][masked] == 0).all()) and bool((got["ds"][masked] == 0).all()), "a masked edge: exact zeros for every head"
        assert bool((got["lse"][dead] == -np.inf).all()) and bool((got["O"][dead] == 0).all()) and bool((got["dQ"][dead] == 0).all())
        assert all(bool(got[k].isfinite().all()) for k in KEYS if k != "lse")
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_head_through_the_new_symbols_equals_the_old_symbols(crp, gpu, dtype):
    """heads = 1 never reaches the new symbols through the wrappers: called directly, they give the single-head calls' bits"""
    import torch
    lib = crp.load()
    sfx = "f64" if dtype == "float64" else "f32"
    rp, ci = _matrix()
    nrow, ncol, nnz = R.NROW, R.NCOL, ci.size
    A, At = _handles(rp, ci, nrow, ncol)
    for dk, dv in (INSTANCES[dtype][8], INSTANCES[dtype][16], (33, 33)):
        Q, K, V, dO, scale = _operands(gpu, dtype, nrow, ncol, 1, dk, dv, 9)
        want = _single(A, At, gpu, Q, K, V, dO, 1, scale)
        O, dQ, dK, dV = _nan(gpu, Q, nrow, dv), _nan(gpu, Q, nrow, dk), _nan(gpu, Q, ncol, dk), _nan(gpu, Q, ncol, dv)
        lse, delta, p, ds = _nan(gpu, Q, nrow, 1), _nan(gpu, Q, nrow, 1), _nan(gpu, Q, nnz, 1), _nan(gpu, Q, nnz, 1)
        P = lambda t: t.data_ptr()
        rc = getattr(lib, "crp_attention_mh_csr_" + sfx)(A.handle, 1, dk, dv, scale, 0, P(Q), dk, P(K), dk, None, 0, P(V), dv, None, 0, P(O),
                                                         dv, P(lse), P(p), None, None)
        assert rc == 0
        rc = getattr(lib, "crp_attention_bwd_q_mh_csr_" + sfx)(A.handle, 1, dk, dv, scale, 0, P(Q), dk, P(K), dk, None, 0, P(V), dv, None, 0,
                                                               P(O), dv, P(dO), dv, P(lse), P(dQ), dk, P(delta), P(ds), None, None)
        assert rc == 0
        rc = getattr(lib, "crp_attention_bwd_kv_mh_csr_" + sfx)(At.handle, 1, dk, dv, scale, 0, P(K), dk, P(V), dv, P(Q), dk, P(dO), dv, P(lse),
                                                                P(delta), P(dK), dk, P(dV), dv, None)
        assert rc == 0
        torch.cuda.synchronize()
        _same(dict(O=O, lse=lse, p=p, dQ=dQ, delta=delta, ds=ds, dK=dK, dV=dV), want, (dtype, dk, dv, "heads = 1"))
    A.free()
    At.free()


@functools.lru_cache(maxsize=None)
def _anchor_case(dtype):
    """H = 3 heads of (24, 20) columns on attention_ref.matrix() as numpy arrays, and attention_ref.reference per head"""
    rp, ci = R.matrix()
    H, dk, dv = 3, 24, 20
    Q, K, V, scale = R.operands(H * dk, H * dv, dtype, 401)
    scale = float(np.dtype(dtype).type(1.0 / np.sqrt(dk)))
    refs = [R.reference(rp, ci, Q[:, h * dk:(h + 1) * dk], K[:, h * dk:(h + 1) * dk], V[:, h * dv:(h + 1) * dv], scale) for h in range(H)]
    return rp, ci, H, dk, dv, Q, K, V, scale, refs


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_reference_per_head(crp, gpu, dtype):
    """an anchor that does not go through the single-head kernels: every entry of O, lse and p_out of every head inside the bound
    of DESIGN.md 5j for (dtype, dk, dv) against the np.longdouble reference on that head's columns"""
    import torch
    from crp_spmm_amd import hip
    rp, ci, H, dk, dv, Q, K, V, scale, refs = _anchor_case(dtype)
    A = hip.CsrDev(R.NROW, R.NCOL, rp, ci, np.ones(ci.size))
    Qd, Kd, Vd = (torch.from_numpy(x).to(gpu) for x in (Q, K, V))
    lse, p = _nan(gpu, Qd, R.NROW, H), _nan(gpu, Qd, ci.size, H)
    O = A.attention(Qd, Kd, Vd, scale=scale, lse=lse, p_out=p, heads=H)
    torch.cuda.synchronize()
    O, lse, p = O.cpu().numpy(), lse.cpu().numpy(), p.cpu().numpy()
    for h in range(H):
        _check((O[:, h * dv:(h + 1) * dv], lse[:, h], p[:, h]), refs[h], dtype, ("multi-head against the reference", dtype, "head %d" % h))
    A.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_attention_with_heads(crp, gpu, dtype):
    """hip.sparse_attention(heads = H): O and the gradients of Q, K, V are the per-head single-head sparse_attention's side by side"""
    import torch
    from crp_spmm_amd import hip
    rp, ci = _matrix()
    A, At = _handles(rp, ci, R.NROW, R.NCOL)
    H = 3
    dk, dv = INSTANCES[dtype][16]
    Q, K, V, dO, scale = _operands(gpu, dtype, R.NROW, R.NCOL, H, dk, dv, 33)
    Qg, Kg, Vg = (t.clone().requires_grad_(True) for t in (Q, K, V))
    O = hip.sparse_attention(A, At, Qg, Kg, Vg, scale=scale, heads=H)
    O.backward(dO)
    torch.cuda.synchronize()
    for h in range(H):
        sk, sv = slice(h * dk, (h + 1) * dk), slice(h * dv, (h + 1) * dv)
        Qh, Kh, Vh = (t.clone().requires_grad_(True) for t in (Q[:, sk], K[:, sk], V[:, sv]))
        Oh = hip.sparse_attention(A, At, Qh, Kh, Vh, scale=scale)
        Oh.backward(dO[:, sv].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(O.detach()[:, sv], Oh.detach()), (dtype, h, "O")
        for name, g, gh, s in (("dQ", Qg.grad, Qh.grad, sk), ("dK", Kg.grad, Kh.grad, sk), ("dV", Vg.grad, Vh.grad, sv)):
            assert torch.equal(g[:, s], gh), (dtype, h, name)
    A.free()
    At.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_error_codes_that_need_a_live_handle(crp, gpu, dtype):
    """-4 for a leading dimension below heads * dk or heads * dv; CRP_ATTN_BWD_EWIDTH for a per-head width over the cap (dk = cap + W
    with H = 2), with nothing written; the same total width 2 (cap + W) in 4 heads runs and equals the single-head calls"""
    import torch
    lib = crp.load()
    tdt = _tdt(dtype)
    sfx = "f64" if dtype == "float64" else "f32"
    cap = B.CAP[np.dtype(dtype)]
    rp, ci, _, _, _, _, _, _ = R.steep_case(dtype)
    nrow, ncol, nnz = rp.size - 1, 80, ci.size
    A, At = _handles(rp, ci, nrow, ncol)
    ffw, fq, fkv = (getattr(lib, "crp_attention_%smh_csr_%s" % (k, sfx)) for k in ("", "bwd_q_", "bwd_kv_"))
    P = lambda t: t.data_ptr()

    def calls(H, dk, dv, ldq=None, ldv=None, heads=None):
        """the three calls on ones, outputs full of a sentinel -> (return codes, outputs); heads: what the calls are told (else H)"""
        wk, wv = H * dk, H * dv
        told = H if heads is None else heads
        ldq, ldv = (wk if ldq is None else ldq), (wv if ldv is None else ldv)
        Q, K, V, O = (torch.ones(s, dtype=tdt, device=gpu) for s in ((nrow, wk), (ncol, wk), (ncol, wv), (nrow, wv)))
        lse_in = torch.zeros((nrow, H), dtype=tdt, device=gpu)
        outs = [torch.full(s, SENT, dtype=tdt, device=gpu) for s in ((nrow, wv), (nrow, H), (nnz, H), (nrow, wk), (nrow, H), (nnz, H), (ncol, wk),
                                                                      (ncol, wv))]
        Oo, lse, p, dQ, delta, ds, dK, dV = outs
        rcs = (ffw(A.handle, told, dk, dv, 1.0, 0, P(Q), ldq, P(K), wk, None, 0, P(V), ldv, None, 0, P(Oo), wv, P(lse), P(p), None, None),
               fq(A.handle, told, dk, dv, 1.0, 0, P(Q), ldq, P(K), wk, None, 0, P(V), ldv, None, 0, P(O), wv, P(O), wv, P(lse_in), P(dQ), wk, P(delta),
                  P(ds), None, None),
               fkv(At.handle, told, dk, dv, 1.0, 0, P(K), wk, P(V), ldv, P(Q), ldq, P(O), wv, P(lse_in), P(lse_in), P(dK), wk, P(dV), wv, None))
        torch.cuda.synchronize()
        return rcs, outs
    untouched = lambda outs: all(bool((t == SENT).all()) for t in outs)
    rcs, outs = calls(2, 8, 8, ldq=15)
    assert rcs == (-4, -4, -4) and untouched(outs), rcs
    rcs, outs = calls(2, 8, 8, ldv=15)
    assert rcs == (-4, -4, -4) and untouched(outs), rcs
    for heads in (0, -2):
        rcs, outs = calls(2, 8, 8, heads=heads)
        assert rcs == (-1, -1, -1) and untouched(outs), rcs
    rcs, outs = calls(2, 8, 8)
    assert rcs == (0, 0, 0) and not any(bool((t == SENT).any()) for t in outs), rcs
    w = W[dtype]
    rcs, outs = calls(2, cap + w, 8)                                # (the forward has no cap)
    assert rcs[0] == 0 and rcs[1:] == (B.EWIDTH, B.EWIDTH) and untouched(outs[3:]), rcs
    rcs, outs = calls(2, 8, cap + w)
    assert rcs[0] == 0 and rcs[1:] == (B.EWIDTH, B.EWIDTH) and untouched(outs[3:]), rcs
    # the wrappers refuse the same before the library; with 4 heads the same total width is served
    H, dk, dv = 2, cap + w, 8
    Q, K, V, dO, scale = _operands(gpu, dtype, nrow, ncol, H, dk, dv, 4)
    lse = torch.zeros((nrow, H), dtype=tdt, device=gpu)
    with pytest.raises(ValueError):
        A.attention_bwd_q(Q, K, V, dO, dO, lse, heads=H)
    with pytest.raises(ValueError):
        At.attention_bwd_kv(K, V, Q, dO, lse, lse, heads=H)
    H, dk, dv = 4, (cap + w) // 2, 4
    assert dk <= cap and dk * 4 == 2 * (cap + w)
    V, dO = V[:, :H * dv].contiguous(), dO[:, :H * dv].contiguous()
    _same(_multi(A, At, gpu, Q, K, V, dO, H, scale), _single(A, At, gpu, Q, K, V, dO, H, scale), (dtype, "4 heads of", dk))
    A.free()
    At.free()
