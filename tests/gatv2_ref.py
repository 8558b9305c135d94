"""Reference, error bound, CPU replay and test data of the fused GATv2 attention over a CSR pattern (csrc/gatv2_kernels.hip):

    z_pj = XT[i]_h[j] + XS[c_p]_h[j],  r_pj = z_pj > 0 ? z_pj : slope z_pj,  s_p = sum_j a_h[j] r_pj (+ val_p),
    O[i]_h = sum_p softmax_p(s) XS[c_p]_h

and of its backward: p = exp(s - lse), dP = <dO[i]_h, XS[c]_h>, D = <dO[i]_h, O[i]_h>, dS = p (dP - D), ag_pj = z_pj > 0 ? a_j : a_j slope;
dXT[i]_h[j] = sum_row dS ag,  da_part[i]_h[j] = sum_row dS r,  dXS[c]_h[j] = sum_column dS ag + sum_column p dO[i]_h[j],
da = the column sums of da_part.

From the scores on the kernels follow the fused attention's order (csrc/attention_kernels.hip, attention_bwd_kernels.hip), so the
forward, delta, dS and the dV-like sum are attention_ref / attention_bwd_ref on a zero dot (Q = K = 0, one column) with the score
as the bias and XS_h as V; what is this file's own is the score, its error D, and the chains over ag and r.

Bound (derived in DESIGN.md 5p, not measured; u = 2^-53 / 2^-24; the reference is np.longdouble on the dtype-rounded XT, XS, a, dO,
values and slope).  The sign of fl(xt + xs) is the sign of xt + xs, so kernel and reference take the same branch and the same g:

    D = max_p u ((dv + 2) sum_j |a_j r_pj| + [bias] |s_p|)     z and slope z: (1 + u)^2 - 1 on every |a_j r_j|; the dot of dv terms:
                                                               dv u sum |a_j r_j|; the bias addition: u |s|

replaces 5j's D in c = (2 L + 4 T + 10 R + 9) u + 2 D; the bounds of O, p_out, lse (5j) and of delta, ds_out (5l, with this c and D
and XS_h as V) keep their form.  With e_S(i) and e_p(i) of 5l and S_p >= |dS_p|:

    |dXT_ij - ref|     <= 1.01 (e_S(i) + (L_i + 1) u) sum_row S_p |ag_pj|         an FMA chain of L terms; as = fl(a slope): one u
    |da_part_ij - ref| <= 1.01 (e_S(i) + (L_i + 2) u) sum_row S_p |r_pj|          r carries two roundings
    |dXS_cj - ref|     <= 1.01 [ sum_column (e_S(i_p) + (Lc + 1) u) S_p |ag_pj|   the dK-like chain
                                 + sum_column (e_p(i_p) + Lc u) p_p |dO[i_p][j]|  the dV-like chain (5l)
                                 + u (sum_column S_p |ag_pj| + sum_column p_p |dO[i_p][j]|) ]      the one addition
    |da_j - ref|       <= sum_i bound(da_part_ij) + 1.01 (255 + ceil(nrow / 256)) u sum_i sum_row S_p |r_pj|

replay() repeats the kernels' FIXED ORDER in numpy: z and r rounded one by one in the dtype, the SDDMM's dot of a with r
(attention_ref.dots_replay), then attention_ref.replay and attention_bwd_ref.replay on those scores, then the FMA chains over ag
and r and col_sum_replay.  numpy's exp is not the device library's, so the replay shows that the ORDER meets the bound and does not
predict the device's bits; col_sum_replay is pure additions and does."""
import functools

import numpy as np

import attention_bwd_ref as B
import attention_ref as R
import gat_ref as G
import softmax_ref as SR

U = SR.U
worst = SR.worst
W = G.W
FWD_KEYS = ("O", "lse", "p")
BWD_KEYS = ("delta", "ds", "dXT", "da_part", "dXS", "da")
CAP = B.CAP
EWIDTH = -6                              # CRP_GATV2_EWIDTH
COL_SUM_ROWS = 256


def _zeros(n, dt):
    return np.zeros((n, 1), dt)


# ---- the scores -------------------------------------------------------------------------------------------------------

def scores_exact(rp, ci, XT, XS, a, slope, h, val=None):
    """(s, mag, r, ag) of head h in np.longdouble from the dtype-rounded inputs (slope rounded to the dtype once): the score per
    nonzero, sum_j |a_j r_j|, and r and ag per nonzero and column"""
    dt = XT.dtype
    H = a.shape[0]
    dv = XT.shape[1] // H
    sv = slice(h * dv, (h + 1) * dv)
    rows = R.rows_of(rp)
    ld = np.longdouble
    sl = ld(dt.type(slope))
    al = a[h].astype(ld)
    z = XT[rows, sv].astype(ld) + XS[ci, sv].astype(ld)
    r = np.where(z > 0, z, sl * z)
    ag = np.where(z > 0, al[None, :], (al * sl)[None, :])
    t = al[None, :] * r
    s, mag = t.sum(axis=1), np.abs(t).sum(axis=1)
    if val is not None:
        s = s + val.astype(dt).astype(ld)
    return s, mag, r, ag


def lrelu_dtype(XT, XS, rows, ci, sv, slope):
    """(z, r) per nonzero and column of one head as the kernels form them: each rounded to the dtype on its own"""
    dt = XT.dtype
    sl = dt.type(slope)
    z = (XT[rows, sv] + XS[ci, sv]).astype(dt)
    r = np.where(z > 0, z, (sl * z).astype(dt)).astype(dt)
    return z, r


def scores_dtype(rp, ci, XT, XS, a, slope, h, val=None):
    """(s, z, r) of head h as the kernels form them: r, then the SDDMM's dot of a_h with r on G(dv) lanes, then + val"""
    dt = XT.dtype
    H = a.shape[0]
    dv = XT.shape[1] // H
    sv = slice(h * dv, (h + 1) * dv)
    rows = R.rows_of(rp)
    z, r = lrelu_dtype(XT, XS, rows, ci, sv, slope)
    lpr = R.group_of(dv, dt)
    s = np.empty(ci.size, dt)
    for b in range(0, ci.size, 2048):
        rb = r[b:b + 2048]
        s[b:b + 2048] = R.dots_replay(np.broadcast_to(a[h][None, :], rb.shape).astype(dt), rb, lpr)
    if val is not None:
        with np.errstate(invalid="ignore"):
            s = (s + val.astype(dt)).astype(dt)
    return s, z, r


# ---- the reference and the bound --------------------------------------------------------------------------------------

def reference(rp, ci, XT, XS, a, slope, val=None, dO=None):
    """name -> (np.longdouble reference, bound), each shaped as the kernels' output: O (rows, H dv), lse (rows, H), p (nnz, H) and,
    with dO, delta (rows, H), ds (nnz, H), dXT, da_part (rows, H dv), dXS (columns, H dv), da (H dv); also "T": the widest spread.
    a: (H, dv)"""
    dt = XT.dtype
    u = U[dt]
    nrow, ncol, nnz, H = rp.size - 1, XS.shape[0], ci.size, a.shape[0]
    dv = XT.shape[1] // H
    ld = np.longdouble
    out = {k: (np.zeros(s, ld), np.zeros(s, ld)) for k, s in (("O", (nrow, H * dv)), ("lse", (nrow, H)), ("p", (nnz, H)))}
    if dO is not None:
        out.update({k: (np.zeros(s, ld), np.zeros(s, ld)) for k, s in (("delta", (nrow, H)), ("ds", (nnz, H)), ("dXT", (nrow, H * dv)),
                                                                          ("da_part", (nrow, H * dv)), ("dXS", (ncol, H * dv)),
                                                                          ("da", (H * dv,)))})
    T = 0.0
    lens = np.diff(rp)
    ne = np.flatnonzero(lens > 0)
    nblk = -(-nrow // COL_SUM_ROWS)
    for h in range(H):
        sv = slice(h * dv, (h + 1) * dv)
        s, mag, r, ag = scores_exact(rp, ci, XT, XS, a, slope, h, val)
        with np.errstate(invalid="ignore"):
            derr = np.where(np.isfinite(s), (dv + 2) * mag + (np.abs(s) if val is not None else 0), 0)
        Vh = np.ascontiguousarray(XS[:, sv])
        if dO is None:
            fwd = R.reference(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), Vh, 1.0, s)
        else:
            bw = B.reference(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), Vh, np.ascontiguousarray(dO[:, sv]), 1.0, s, ncol=ncol)
            fwd = bw["fwd"]
        fwd["D"] = np.zeros(nrow, ld)
        if ne.size:
            fwd["D"][ne] = np.maximum.reduceat(derr, rp[ne].astype(np.intp))
        T = max(T, float(fwd["T"].max()) if nrow else 0.0)
        for k, ref, bnd in (("O", fwd["O"], R.bound_O(fwd, dt)), ("lse", fwd["lse"], R.bound_lse(fwd, dt)), ("p", fwd["p"], R.bound_p(fwd, dt))):
            sel = sv if k == "O" else h
            out[k][0][:, sel], out[k][1][:, sel] = ref, bnd
        if dO is None:
            continue
        e_p, e_S = B.coeffs(bw, dt)
        tm, cit, rpt = bw["tmap"], bw["cit"], bw["rpt"]
        Lc = np.diff(rpt).astype(np.float64)[R.rows_of(rpt)]
        ds, S, L = bw["ds"], bw["S"], fwd["L"]
        absag, absr = np.abs(ag), np.abs(r)
        dXT = B._seg_sum(ds[:, None] * ag, rp)
        dap = B._seg_sum(ds[:, None] * r, rp)
        MX, MA = B._seg_sum(S[:, None] * absag, rp), B._seg_sum(S[:, None] * absr, rp)
        b_dXT = 1.01 * (e_S + (L + 1) * u)[:, None] * MX
        b_dap = 1.01 * (e_S + (L + 2) * u)[:, None] * MA
        accZ = B._seg_sum(ds[tm, None] * ag[tm], rpt)
        MZ = B._seg_sum(S[tm, None] * absag[tm], rpt)
        MV = B._seg_sum(bw["p"][tm, None] * bw["absdO"][cit], rpt)
        b_Z = 1.01 * B._seg_sum(((e_S[cit] + (Lc + 1) * u) * S[tm])[:, None] * absag[tm], rpt)
        b_dXS = b_Z + B.bound_dV(bw, dt) + 1.01 * u * (MZ + MV)
        da = dap.sum(axis=0)
        b_da = b_dap.sum(axis=0) + 1.01 * (COL_SUM_ROWS - 1 + nblk) * u * MA.sum(axis=0)
        out["da"][0][sv], out["da"][1][sv] = da, b_da
        for k, ref, bnd in (("delta", bw["delta"], B.bound_delta(bw, dt)), ("ds", ds, B.bound_ds(bw, dt)), ("dXT", dXT, b_dXT),
                            ("da_part", dap, b_dap), ("dXS", accZ + bw["dV"], b_dXS)):
            sel = sv if k in ("dXT", "da_part", "dXS") else h
            out[k][0][:, sel], out[k][1][:, sel] = ref, bnd
    out["T"] = T
    return out


def ratios(got, ref):
    """worst |got - ref| / bound per output of `got` (name -> array); lse: -inf must match exactly and is left out of the ratio"""
    return G.ratios(got, ref)


# ---- the replay -------------------------------------------------------------------------------------------------------

def col_sum_replay(x):
    """crp_col_sum_*'s order on a 2-D array, in its dtype: blocks of 256 rows from +0 in ascending row, then the blocks left to right
    starting from the first block's sum (no rows: +0)"""
    dt = x.dtype
    nrow, n = x.shape
    if nrow == 0:
        return np.zeros(n, dt)
    tot = None
    for b in range(0, nrow, COL_SUM_ROWS):
        acc = np.zeros(n, dt)
        for r in range(b, min(nrow, b + COL_SUM_ROWS)):
            acc = (acc + x[r]).astype(dt)
        tot = acc if tot is None else (tot + acc).astype(dt)
    return tot


def replay(rp, ci, XT, XS, a, slope, val=None, dO=None, exp=np.exp):
    """name -> array in the operands' dtype, in the kernels' order (the keys of reference())"""
    dt = XT.dtype
    nrow, ncol, nnz, H = rp.size - 1, XS.shape[0], ci.size, a.shape[0]
    dv = XT.shape[1] // H
    out = dict(O=np.zeros((nrow, H * dv), dt), lse=np.zeros((nrow, H), dt), p=np.zeros((nnz, H), dt))
    if dO is not None:
        out.update(delta=np.zeros((nrow, H), dt), ds=np.zeros((nnz, H), dt), dXT=np.zeros((nrow, H * dv), dt),
                   da_part=np.zeros((nrow, H * dv), dt), dXS=np.zeros((ncol, H * dv), dt))
        rpt, cit, tmap = B.transpose(rp, ci, ncol)
    sl = dt.type(slope)
    every = np.arange(nnz)
    for h in range(H):
        sv = slice(h * dv, (h + 1) * dv)
        s, z, r = scores_dtype(rp, ci, XT, XS, a, slope, h, val)
        Vh = np.ascontiguousarray(XS[:, sv])
        O, lse, p = R.replay(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), Vh, 1.0, s, exp=exp)
        out["O"][:, sv], out["lse"][:, h], out["p"][:, h] = O, lse, p
        if dO is None:
            continue
        bw = B.replay(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), Vh, O, lse, np.ascontiguousarray(dO[:, sv]), 1.0, s, exp=exp)
        ah = a[h].astype(dt)
        ag = np.where(z > 0, ah[None, :], (ah * sl).astype(dt)[None, :]).astype(dt)
        ds = bw["ds"]
        out["delta"][:, h], out["ds"][:, h] = bw["delta"], ds
        out["dXT"][:, sv] = B._chain(rp, ds, ag, every)
        out["da_part"][:, sv] = B._chain(rp, ds, r, every)
        out["dXS"][:, sv] = (B._chain(rpt, ds[tmap], ag, tmap) + bw["dV"]).astype(dt)
    if dO is not None:
        out["da"] = col_sum_replay(out["da_part"])
    return out


# ---- test data --------------------------------------------------------------------------------------------------------

NROW, NCOL, K0, EMPTY_COL = G.NROW, G.NCOL, G.K0, G.EMPTY_COL
SPREADS = G.SPREADS
SLOPE = G.SLOPE
SHORT = 9                                # rows of at most this many entries make the pattern of the wide cases
matrix = G.matrix
two_source_codes = G.two_source_codes


@functools.lru_cache(maxsize=None)
def short_matrix():
    """(rp, ci, rows): the rows of matrix() of at most SHORT entries, in order, and which rows they are"""
    rp, ci = G.matrix()
    lens = np.diff(rp)
    keep = np.flatnonzero(lens <= SHORT)
    sel = (lens <= SHORT)[R.rows_of(rp)]
    rps = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int32)
    cis = ci[sel].copy()
    assert set(lens[keep]) >= {0, 1, 7, 8, 9}
    rps.setflags(write=False)
    cis.setflags(write=False)
    return rps, cis, keep


def operands(dtype, H, dv, spread, seed, nrow=NROW, ncol=NCOL):
    """XT, XS, a (H, dv), dO in the dtype: standard normal; a times spread / sqrt(dv), so that `spread` is the scale of the scores
    whatever the width"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    XT = rng.standard_normal((nrow, H * dv)).astype(dt)
    XS = rng.standard_normal((ncol, H * dv)).astype(dt)
    a = (spread / np.sqrt(dv) * rng.standard_normal((H, dv))).astype(dt)
    dO = rng.standard_normal((nrow, H * dv)).astype(dt)
    return XT, XS, a, dO


def widths(dtype):
    """one head's widths: gat_ref's (1, 5, the last of the group of 8 lanes and the first past it, one past 32 W and past 64 W)"""
    return G.widths(dtype)


def cap(dtype):
    return CAP[np.dtype(dtype)]


def bound_cases():
    """(dtype, H, dv, spread, short): what test_gpu_gatv2.py holds against the bound and test_gatv2_ref.py replays; the cap runs on
    the rows of at most SHORT entries"""
    for dtype in ("float64", "float32"):
        for i, dv in enumerate(widths(dtype)):
            for H in (1, 3):
                yield dtype, H, dv, SPREADS[(i + H) % 2], False
        for H in (1, 3):
            yield dtype, H, cap(dtype), SPREADS[H % 2], True


@functools.lru_cache(maxsize=None)
def case(dtype, H, dv, spread, short=False):
    """(rp, ci, XT, XS, a, dO, ref) of one bound case, computed once and read-only"""
    dt = np.dtype(dtype)
    if short:
        rp, ci, _ = short_matrix()
    else:
        rp, ci = G.matrix()
    XT, XS, a, dO = operands(dt, H, dv, spread, 2000 * H + dv + (dt == np.float32), nrow=rp.size - 1)
    ref = reference(rp, ci, XT, XS, a, SLOPE, None, dO)
    assert ref["T"] <= SR.T_MAX[dt], ref["T"]            # 5j's data rule, before anything else
    for x in (XT, XS, a, dO):
        x.setflags(write=False)
    return rp, ci, XT, XS, a, dO, ref


def chunk_widths(dtype):
    """gat_ref.chunk_widths up to the cap: either side of 16 W, 32 W, 64 W and 128 W, 17 W + 1, 40 W + 1 and the cap"""
    return G.chunk_widths(dtype, "gatv2")


def chunk_bound_cases():
    """(dtype, H, dv, spread) on gat_ref.chunk_matrix(): H = 3 and H = 1 on the widths up to 64 W + 1, H = 1 above (the reference's
    cost grows with H dv)"""
    for dtype in ("float64", "float32"):
        w = W[dtype]
        for i, dv in enumerate(chunk_widths(dtype)):
            for H in ((1, 3) if dv <= 64 * w + 1 else (1,)):
                yield dtype, H, dv, SPREADS[(i + H) % 2]


@functools.lru_cache(maxsize=None)
def chunk_case(dtype, H, dv, spread):
    """(rp, ci, XT, XS, a, dO, ref) of one bound case on gat_ref.chunk_matrix(), computed once and read-only"""
    dt = np.dtype(dtype)
    rp, ci = G.chunk_matrix()
    XT, XS, a, dO = operands(dt, H, dv, spread, 4000 * H + dv + (dt == np.float32), nrow=G.CHUNK_NROW, ncol=G.CHUNK_NCOL)
    ref = reference(rp, ci, XT, XS, a, SLOPE, None, dO)
    for x in (XT, XS, a, dO):
        x.setflags(write=False)
    return rp, ci, XT, XS, a, dO, ref


@functools.lru_cache(maxsize=None)
def steep_case(dtype, H=3, dv=20):
    """attention_ref.steep_case's rows -- ascending, descending, late-peak and half-masked, T up to 60 -- with its bias as the
    matrix's values (bias = 1) under small scores of its own: (rp, ci, val, XT, XS, a, dO, ref); 80 columns"""
    dt = np.dtype(dtype)
    rp, ci, val = R.steep_case(dtype)[:3]
    XT, XS, a, dO = operands(dt, H, dv, 0.25, 91, nrow=rp.size - 1, ncol=80)
    ref = reference(rp, ci, XT, XS, a, SLOPE, val, dO)
    assert 40 < ref["T"] <= SR.T_MAX[dt], ref["T"]
    return rp, ci, val, XT, XS, a, dO, ref


def exact_operands(dtype, H, dv, seed, nrow=NROW, ncol=NCOL):
    """XT, XS, a, dO whose every z, r, product and partial sum of the score is exact under slope 1/4: integers in [-8, 8] for XT
    and XS (z a multiple of 1, slope z a multiple of 1/4, both far below 2^24), a in {-2, ..., 2} / 8 -- so the score is a sum of
    at most 1024 multiples of 1/32 below 2^7, exact in fp32 in any order"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    XT = rng.integers(-8, 9, (nrow, H * dv)).astype(dt)
    XS = rng.integers(-8, 9, (ncol, H * dv)).astype(dt)
    a = (rng.integers(-2, 3, (H, dv)) / 8.0).astype(dt)
    dO = rng.standard_normal((nrow, H * dv)).astype(dt)
    return XT, XS, a, dO
