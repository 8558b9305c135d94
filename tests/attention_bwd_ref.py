"""Reference, error bound, CPU replay and test data of the fused backward of the sparse attention
(csrc/attention_bwd_kernels.hip).  With O and lse as the forward wrote them and the upstream gradient dO, per nonzero p = (i, c):

    s_p = scale <Q[i], K[c]> (+ bias_p),  p_p = exp(s_p - lse[i]),  dP_p = <dO[i], V[c]>,  D_i = <dO[i], O[i]>,  dS_p = p_p (dP_p - D_i)
    dQ[i] = scale sum_{row i} dS_p K[c_p],   dK[c] = scale sum_{column c} dS_p Q[i_p],   dV[c] = sum_{column c} p_p dO[i_p]

The reference is np.longdouble on the dtype-rounded Q, K, V, dO: the exact gradient (its O and lse are exact too).

Bound (derived in DESIGN.md 5l, not measured; u = 2^-53 / 2^-24; L_i the row's length, Lc the column's; c_i, D_i, T_i the
forward's coefficient, score error and spread of row i, tests/attention_ref.py; a_p = sum_j |dO_ij| |V_cj|, Abar_i = sum_q p_q a_q,
S_p = p_p (a_p + Abar_i) >= |dS_p|):

    the kernel's O and lse are inputs with |O - ref| <= bound_O = 1.01 c_i A_ij and |lse - ref| <= bound_lse =: B_i
    e_p(i)  = D_i + B_i + (T_i + log L_i + 4) u          relative error of p_p: the score, lse, the subtraction of two numbers of
                                                         size <= T + log L, and exp within 2 ulp (4 u)
    |delta_i - ref|  <= 1.01 (c_i + nv u) Abar_i         O's error through the dot, and the dot's nv u
    e_S(i)  = e_p(i) + c_i + (nv + 2) u                  dP's dot (nv u a_p), delta's error, the subtraction and the product
    |ds_out_p - ref| <= 1.01 e_S(i) S_p
    |dQ_ij - ref|    <= 1.01 (e_S(i) + (L_i + 1) u) |scale| sum_{row i} S_p |K[c_p][j]|          an FMA chain of L_i terms, times scale
    |dK_cj - ref|    <= 1.01 |scale| sum_{column c} (e_S(i_p) + (Lc + 1) u) S_p |Q[i_p][j]|
    |dV_cj - ref|    <= 1.01 sum_{column c} (e_p(i_p) + Lc u) p_p |dO[i_p][j]|

Data rule: the forward's (T <= 60 in fp32, 600 in fp64, nothing near the subnormal range).

replay() repeats the kernels' FIXED ORDER in numpy (attention_ref.dots_replay for every dot, softmax_ref.fma for every FMA);
numpy's exp is not the device library's, so it shows that the ORDER meets the bound and does not predict the device's bits."""
import functools

import numpy as np

import attention_ref as R
import softmax_ref as SR

U = SR.U
worst = SR.worst
CAP = {np.dtype(np.float64): 512, np.dtype(np.float32): 1024}
EWIDTH = -6                              # CRP_ATTN_BWD_EWIDTH


def transpose(rp, ci, ncol):
    """(rpt, cit, tmap): A^T in the stable transposed order (rows of column c ascending); tmap[q] = position in A of entry q"""
    rows = R.rows_of(rp)
    tmap = np.lexsort((rows, ci)).astype(np.int32)
    rpt = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncol))]).astype(np.int32)
    return rpt, rows[tmap].astype(np.int32), tmap


# ---- the reference ----------------------------------------------------------------------------------------------------

def _seg_sum(t, rp):
    """per row of rp, the sum of the rows of t (2-D, one per nonzero)"""
    out = np.zeros((rp.size - 1,) + t.shape[1:], t.dtype)
    ne = np.flatnonzero(np.diff(rp) > 0)
    if ne.size:
        out[ne] = np.add.reduceat(t, rp[ne].astype(np.intp), axis=0)
    return out


def reference(rp, ci, Q, K, V, dO, scale, bias=None, ncol=None):
    """np.longdouble gradients on the dtype-rounded inputs and what the bounds take.  Returns a dict: fwd (attention_ref's
    reference), dQ, dK, dV, ds, delta and the magnitudes a, Abar, S, MQ = |scale| sum S |K|, MK = |scale| sum S |Q|, MV = sum p |dO|
    (MK, MV per entry weight are formed in the bounds)."""
    ncol = K.shape[0] if ncol is None else ncol
    fwd = R.reference(rp, ci, Q, K, V, scale, bias)
    rows = fwd["rows"]
    sc = np.longdouble(Q.dtype.type(scale))
    p = fwd["p"]
    dOl, Vl, Kl, Ql = (x.astype(np.longdouble) for x in (dO, V, K, Q))
    nnz = ci.size
    dP = np.empty(nnz, np.longdouble)
    a = np.empty(nnz, np.longdouble)
    for b in range(0, nnz, 1024):
        t = dOl[rows[b:b + 1024]] * Vl[ci[b:b + 1024]]
        dP[b:b + 1024] = t.sum(axis=1)
        a[b:b + 1024] = np.abs(t).sum(axis=1)
    delta = _seg_sum((p * dP)[:, None], rp)[:, 0]
    Abar = _seg_sum((p * a)[:, None], rp)[:, 0]
    ds = p * (dP - delta[rows])
    S = p * (a + Abar[rows])
    rpt, cit, tmap = transpose(rp, ci, ncol)
    dQ = sc * _seg_sum(ds[:, None] * Kl[ci], rp)
    dK = sc * _seg_sum(ds[tmap, None] * Ql[cit], rpt)
    dV = _seg_sum(p[tmap, None] * dOl[cit], rpt)
    return dict(fwd=fwd, rows=rows, rp=rp, ci=ci, rpt=rpt, cit=cit, tmap=tmap, scale=abs(sc), nv=V.shape[1], p=p, a=a, Abar=Abar, S=S,
                ds=ds, delta=delta, dQ=dQ, dK=dK, dV=dV, absK=np.abs(Kl), absQ=np.abs(Ql), absdO=np.abs(dOl))


# ---- the bounds -------------------------------------------------------------------------------------------------------

def coeffs(ref, dtype):
    """(e_p, e_S) per row of A, as float64 (see the module's docstring)"""
    u = U[np.dtype(dtype)]
    fwd = ref["fwd"]
    c = R.coeff(fwd, dtype)
    L = fwd["L"]
    e_p = fwd["D"].astype(np.float64) * u + R.bound_lse(fwd, dtype).astype(np.float64) + (fwd["T"] + np.log(np.maximum(L, 1)) + 4) * u
    e_S = e_p + c + (ref["nv"] + 2) * u
    return e_p, e_S


def bound_delta(ref, dtype):
    u = U[np.dtype(dtype)]
    return 1.01 * (R.coeff(ref["fwd"], dtype) + ref["nv"] * u) * ref["Abar"]


def bound_ds(ref, dtype):
    return 1.01 * coeffs(ref, dtype)[1][ref["rows"]] * ref["S"]


def bound_dQ(ref, dtype):
    u = U[np.dtype(dtype)]
    e_S = coeffs(ref, dtype)[1]
    mag = ref["scale"] * _seg_sum(ref["S"][:, None] * ref["absK"][ref["ci"]], ref["rp"])
    return 1.01 * (e_S + (ref["fwd"]["L"] + 1) * u)[:, None] * mag


def bound_dK(ref, dtype):
    u = U[np.dtype(dtype)]
    e_S = coeffs(ref, dtype)[1]
    Lc = np.diff(ref["rpt"]).astype(np.float64)
    tm, cit = ref["tmap"], ref["cit"]
    w = (e_S[cit] + (Lc[R.rows_of(ref["rpt"])] + 1) * u) * ref["S"][tm]
    return 1.01 * ref["scale"] * _seg_sum(w[:, None] * ref["absQ"][cit], ref["rpt"])


def bound_dV(ref, dtype):
    u = U[np.dtype(dtype)]
    e_p = coeffs(ref, dtype)[0]
    Lc = np.diff(ref["rpt"]).astype(np.float64)
    tm, cit = ref["tmap"], ref["cit"]
    w = (e_p[cit] + Lc[R.rows_of(ref["rpt"])] * u) * ref["p"][tm]
    return 1.01 * _seg_sum(w[:, None] * ref["absdO"][cit], ref["rpt"])


def chain_magnitudes(ref):
    """what tests/test_gpu_attention.py::test_one_backward_step_from_the_existing_calls bounds the chain of existing calls
    against, each to be taken 8 * 1.01 * max c times: (dQ, dK, dV)"""
    tm, cit = ref["tmap"], ref["cit"]
    return (ref["scale"] * _seg_sum(ref["S"][:, None] * ref["absK"][ref["ci"]], ref["rp"]),
            ref["scale"] * _seg_sum(ref["S"][tm, None] * ref["absQ"][cit], ref["rpt"]),
            _seg_sum(ref["p"][tm, None] * ref["absdO"][cit], ref["rpt"]))


def ratios(got, ref, dtype):
    """worst |got - ref| / bound of dQ, dK, dV, ds_out, delta; got: a dict with some of those keys"""
    bounds = dict(dQ=bound_dQ, dK=bound_dK, dV=bound_dV, ds=bound_ds, delta=bound_delta)
    out = {}
    for k, v in got.items():
        if v is None:
            continue
        assert np.isfinite(v).all(), (k, "non-finite output")
        out[k] = worst(np.asarray(v).ravel(), ref[k].ravel(), np.asarray(bounds[k](ref, dtype)).ravel())[0]
    return out


# ---- the replay -------------------------------------------------------------------------------------------------------

def _chain(rp, coef, rowsrc, idx):
    """per row of rp: acc = fma(coef[p], rowsrc[idx[p]], acc) in ascending p, from +0 (coef == 0 adds exactly nothing)"""
    dt = rowsrc.dtype
    lens = np.diff(rp).astype(np.int64)
    acc = np.zeros((rp.size - 1, rowsrc.shape[1]), dt)
    order = np.argsort(-lens, kind="stable")
    for t in range(int(lens.max()) if lens.size else 0):
        r = order[:int((lens > t).sum())]
        p = rp[r].astype(np.int64) + t
        on = coef[p] != 0
        if on.any():
            r, p = r[on], p[on]
            acc[r] = SR.fma(np.broadcast_to(coef[p, None], (r.size, rowsrc.shape[1])), rowsrc[idx[p]], acc[r])
    return acc


def replay(rp, ci, Q, K, V, O, lse, dO, scale, bias=None, exp=np.exp):
    """dict(dQ, dK, dV, ds, delta) in the operands' dtype, in the kernels' order; O and lse: what the forward wrote, in the dtype"""
    dt = Q.dtype
    nk, nv = Q.shape[1], V.shape[1]
    lpr = R.lpr_of(nk, nv, dt)
    rows = R.rows_of(rp)
    s, _ = R.scores_replay(rp, ci, Q, K, scale, bias, lpr)
    delta = R.dots_replay(dO, O, lpr)
    dP = np.empty(ci.size, dt)
    for b in range(0, ci.size, 2048):
        dP[b:b + 2048] = R.dots_replay(dO[rows[b:b + 2048]], V[ci[b:b + 2048]], lpr)
    dead = np.isneginf(lse)[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        arg = np.where(dead, 0, s - np.where(dead, 0, lse[rows])).astype(dt)
        p = np.where(dead, 0, np.asarray(exp(arg))).astype(dt)
        ds = np.where(p == 0, 0, p * (dP - delta[rows])).astype(dt)
    sc = dt.type(scale)
    rpt, cit, tmap = transpose(rp, ci, K.shape[0])
    dQ = (_chain(rp, ds, K, ci) * sc).astype(dt)
    dK = (_chain(rpt, ds[tmap], Q, cit) * sc).astype(dt)
    dV = _chain(rpt, p[tmap], dO, cit)
    return dict(dQ=dQ, dK=dK, dV=dV, ds=ds, delta=delta, p=p)


# ---- test data --------------------------------------------------------------------------------------------------------

SPECIAL_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 200, 0)
NROW, NCOL = 2048, 640
HUB, EMPTY_COL, ONE_COL, EIGHT_COL, NINE_COL = 5, 17, 18, 19, 20
SHORT = 9                                # rows of at most this many entries make the pattern of the wide cases


@functools.lru_cache(maxsize=None)
def matrix(short=False, seed=13):
    """(rp, ci, nrow): NROW rows over NCOL columns.  The first rows have SPECIAL_LENGTHS, the others 2 .. 6 entries; every row of
    two or more entries names the hub column (> 2000 entries); EMPTY_COL, ONE_COL, EIGHT_COL and NINE_COL have 0, 1, 8 and 9.
    short: the rows of at most SHORT entries among the first 256, as a matrix of their own (the hub has a few hundred)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 7, NROW)
    lens[:len(SPECIAL_LENGTHS)] = SPECIAL_LENGTHS
    lens[120], lens[130:138], lens[140:149] = 4, 5, 3         # the rows that name ONE_COL, EIGHT_COL, NINE_COL
    pool = np.setdiff1d(np.arange(NCOL), [HUB, EMPTY_COL, ONE_COL, EIGHT_COL, NINE_COL])
    cols = []
    for r, n in enumerate(lens):
        n = int(n)
        if n < 2:
            cols.append(rng.choice(pool, size=n, replace=False))
            continue
        extra = ONE_COL if r == 120 else EIGHT_COL if 130 <= r < 138 else NINE_COL if 140 <= r < 149 else None
        own = [HUB] + ([extra] if extra is not None else [])
        cols.append(np.sort(np.concatenate([own, rng.choice(pool, size=n - len(own), replace=False)])))
    if short:
        keep = np.flatnonzero(lens[:256] <= SHORT)
        lens, cols = lens[keep], [cols[r] for r in keep]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci, int(lens.size)


def check_matrix():
    """the properties the tests rely on"""
    rp, ci, nrow = matrix()
    lens, cnt = np.diff(rp), np.bincount(ci, minlength=NCOL)
    assert nrow == NROW and set(SPECIAL_LENGTHS) <= set(lens.tolist())
    assert cnt[HUB] >= 2000 and cnt[EMPTY_COL] == 0 and cnt[ONE_COL] == 1 and cnt[EIGHT_COL] == 8 and cnt[NINE_COL] == 9, cnt[[HUB, 17, 18, 19, 20]]
    rps, cis, ns = matrix(short=True)
    assert np.diff(rps).max() <= SHORT and {0, 1, 7, 8, 9} <= set(np.diff(rps).tolist())


# either side of every instance threshold (fp64: 16/17, 32/33, 64/65, 128/129, 256/257; fp32: twice those) and the cap
WIDTHS = {"float64": ((3, 5), (16, 16), (17, 17), (32, 33), (33, 32), (8, 40), (64, 64), (65, 65), (130, 4), (128, 129), (129, 128),
                      (256, 256), (257, 257), (512, 512)),
          "float32": ((3, 5), (32, 32), (33, 33), (64, 65), (65, 64), (8, 40), (128, 128), (129, 129), (260, 4), (256, 257), (257, 256),
                      (512, 512), (513, 513), (1024, 1024))}
WIDE = {"float64": 130, "float32": 260}      # from here on: the short-row pattern


def parity_cases():
    for dtype in ("float64", "float32"):
        for nk, nv in WIDTHS[dtype]:
            yield nk, nv, dtype


def operands(nk, nv, dtype, seed, nrow=NROW, ncol=NCOL):
    """Q, K, V, dO in the dtype (standard normal) and the scale 1 / sqrt(nk)"""
    Q, K, V, scale = R.operands(nk, nv, dtype, seed, nrow=nrow, ncol=ncol)
    dO = np.random.default_rng(seed + 7).standard_normal((nrow, nv)).astype(dtype)
    return Q, K, V, dO, scale


@functools.lru_cache(maxsize=None)
def case(nk, nv, dtype):
    """(rp, ci, nrow, Q, K, V, dO, scale, ref) of one parity case, computed once and read-only"""
    dt = np.dtype(dtype)
    rp, ci, nrow = matrix(short=max(nk, nv) >= WIDE[dt.name])
    Q, K, V, dO, scale = operands(nk, nv, dt, 100 * nk + nv + (dt == np.float32), nrow=nrow)
    ref = reference(rp, ci, Q, K, V, dO, scale)
    assert ref["fwd"]["T"].max() <= SR.T_MAX[dt]
    for x in (Q, K, V, dO):
        x.setflags(write=False)
    return rp, ci, nrow, Q, K, V, dO, scale, ref


def dense_case(m=64, nk=16, nv=24, seed=5):
    """the pattern and operands of tests/test_gpu_attention.py::test_one_backward_step_from_the_existing_calls (fp64, no empty
    row: torch's softmax of one is NaN): (rp, ci, Q, K, V, dO, scale)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 13, m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(m, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    Q, K, V, scale = R.operands(nk, nv, "float64", 21, nrow=m, ncol=m)
    dO = np.random.default_rng(22).standard_normal((m, nv))
    return rp, ci, Q, K, V, dO, scale


def dense_autograd(rp, ci, Q, K, V, dO, scale):
    """(dQ, dK, dV) by torch autograd on the dense masked attention, on the CPU"""
    import torch
    m, ncol = Q.shape[0], K.shape[0]
    Qt, Kt, Vt = (torch.from_numpy(np.array(x)).requires_grad_(True) for x in (Q, K, V))
    mask = torch.zeros((m, ncol), dtype=torch.bool)
    mask[torch.from_numpy(R.rows_of(rp)), torch.from_numpy(ci.astype(np.int64))] = True
    S = (Qt @ Kt.T) * scale
    P = torch.softmax(S.masked_fill(~mask, float("-inf")), dim=1)
    P = torch.where(mask.any(dim=1, keepdim=True), P, torch.zeros_like(P))
    (P @ Vt).backward(torch.from_numpy(np.array(dO)))
    return Qt.grad.numpy(), Kt.grad.numpy(), Vt.grad.numpy()
