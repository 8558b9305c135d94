"""Reference, error bound, CPU replay and test data of the fused sparse attention over a CSR pattern
(csrc/attention_kernels.hip):  s_p = scale <Q[i], K[c_p]> (+ bias_p),  O[i] = sum_p softmax_p(s) V[c_p].

Bound (derived in DESIGN.md 5j, not measured; u = 2^-53 / 2^-24, L the row's length, R = ceil(L / 8) its batches,
T = max (m - s) over the row's finite scores; the reference is np.longdouble on the dtype-rounded inputs):

    D   = max_p u ((nk + 1) |scale| sum_j |q_j k_pj| + [bias] |s_p|)          the scores' error: it shifts every exponent
    c   = (2 L + 4 T + 10 R + 9) u + 2 D                                     per row
    |O_j - ref|   <= 1.01 c sum_p p_p |V[c_p][j]|
    |p_p - ref|   <= 1.01 c p_p
    |lse - ref|   <= 1.01 (c + 4 u |log l| + u (|m| + |lse|))

replay() repeats the kernel's FIXED ORDER in numpy: the SDDMM's dot (column j in lane (j / W) % LPR, per-lane FMA chains in
ascending j, the balanced binary tree over the lanes), s = dot * scale (+ bias), batches of 8 with m' = max(m, batch),
f = exp(m - m'), e = exp(s - m'), l = l f + e_0 + ... + e_7 left to right, acc = acc f, then FMAs in ascending u; O = acc / l.
FMAs are softmax_ref.fma (one rounding).  numpy's exp is not the device library's, so the replay shows that the ORDER meets the
bound and does not predict the device's bits."""
import functools

import numpy as np

import softmax_ref as SR

U = SR.U
UNR = 8


def group_of(n, dtype):
    """the SDDMM's lane group for a width n (csrc/sddmm_kernels.hip)"""
    w = 16 // np.dtype(dtype).itemsize
    return 8 if n <= 8 * w else 16 if n <= 16 * w else 32 if n <= 32 * w else 64


def lpr_of(nk, nv, dtype):
    """the attention kernel's lane group (csrc/attention_kernels.hip, INSTANCE)"""
    return max(group_of(nk, dtype), group_of(nv, dtype))


def instance_of(nk, nv, dtype):
    """(LPR, PK, PV) of the kernel instance"""
    w = 16 // np.dtype(dtype).itemsize
    lpr = lpr_of(nk, nv, dtype)
    if lpr < 64:
        return lpr, 1, 1
    pk = 1 if nk <= 64 * w else 2 if nk <= 128 * w else 4 if nk <= 256 * w else 0
    pv = 1 if nv <= 64 * w else 2 if nv <= 128 * w else 4 if nv <= 256 * w else 8
    return lpr, pk, pv


def rows_of(rp):
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def _rows_of_codes(ci, K0, K1):
    """rows of the two-source operand by column code (K1 None: one source)"""
    if K1 is None:
        return K0[ci]
    out = np.empty((ci.size, K0.shape[1]), K0.dtype)
    pos = ci >= 0
    out[pos] = K0[ci[pos]]
    out[~pos] = K1[~ci[~pos]]
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------

def reference(rp, ci, Q, K, V, scale, bias=None, chunk=1024):
    """np.longdouble results on the dtype-rounded inputs (K, V: one source, indexed by ci; scale already rounded to the dtype;
    bias: None or the values per nonzero in the dtype, -inf = masked).  Returns a dict: O, A = sum_p p_p |V|, p, lse, and per
    row L, T, D / u (the scores' error in units of u) -- what bound() takes."""
    dt = Q.dtype
    nrow, nnz, nk, nv = rp.size - 1, ci.size, Q.shape[1], V.shape[1]
    rows = rows_of(rp)
    sc = np.longdouble(dt.type(scale))
    s = np.empty(nnz, np.longdouble)
    S = np.empty(nnz, np.longdouble)
    Ql, Kl = Q.astype(np.longdouble), K.astype(np.longdouble)
    for a in range(0, nnz, chunk):
        prod = Ql[rows[a:a + chunk]] * Kl[ci[a:a + chunk]]
        s[a:a + chunk] = sc * prod.sum(axis=1)
        S[a:a + chunk] = abs(sc) * np.abs(prod).sum(axis=1)
    derr = (nk + 1) * S
    if bias is not None:
        s = s + bias.astype(np.longdouble)
        with np.errstate(invalid="ignore"):
            derr = derr + np.where(np.isfinite(s), np.abs(s), 0)
    lens = np.diff(rp)
    ne = np.flatnonzero(lens > 0)
    starts = rp[ne].astype(np.intp)
    m = np.full(nrow, -np.inf, np.longdouble)
    if ne.size:
        m[ne] = np.maximum.reduceat(s, starts)
    with np.errstate(invalid="ignore"):
        d = m[rows] - s
        fin = np.isfinite(d)
        e = np.where(fin, np.exp(-np.where(fin, d, 0)), 0).astype(np.longdouble)
    tot = np.zeros(nrow, np.longdouble)
    T = np.zeros(nrow)
    D = np.zeros(nrow, np.longdouble)
    if ne.size:
        tot[ne] = np.add.reduceat(e, starts)
        T[ne] = np.maximum.reduceat(np.where(fin, d, 0).astype(np.float64), starts)
        D[ne] = np.maximum.reduceat(np.where(fin, derr, 0), starts)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.where(tot[rows] > 0, e / tot[rows], 0).astype(np.longdouble)
        lse = np.where(tot > 0, m + np.log(np.where(tot > 0, tot, 1)), -np.inf)
    O = np.zeros((nrow, nv), np.longdouble)
    A = np.zeros((nrow, nv), np.longdouble)
    Vl = V.astype(np.longdouble)
    for j in range(0, nv, 64):
        if ne.size:
            t = p[:, None] * Vl[ci, j:j + 64]
            O[ne, j:j + 64] = np.add.reduceat(t, starts, axis=0)
            A[ne, j:j + 64] = np.add.reduceat(np.abs(t), starts, axis=0)
    return dict(O=O, A=A, p=p, lse=lse, m=m, tot=tot, L=lens.astype(np.float64), T=T, D=D, rows=rows)


def coeff(ref, dtype):
    """c per row (see the module's docstring)"""
    u = U[np.dtype(dtype)]
    L = ref["L"]
    return ((2 * L + 4 * ref["T"] + 10 * np.ceil(L / UNR) + 9) + 2 * ref["D"].astype(np.float64)) * u


def bound_O(ref, dtype):
    return 1.01 * coeff(ref, dtype)[:, None] * ref["A"]


def bound_p(ref, dtype):
    return 1.01 * coeff(ref, dtype)[ref["rows"]] * ref["p"]


def bound_lse(ref, dtype):
    u = U[np.dtype(dtype)]
    live = ref["tot"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        extra = np.where(live, 4 * np.abs(np.log(np.where(live, ref["tot"], 1))) + np.abs(ref["m"]) + np.abs(ref["lse"]), 0)
    return 1.01 * (coeff(ref, dtype) + u * extra.astype(np.float64))


# ---- the replay -------------------------------------------------------------------------------------------------------

def dots_replay(q, k, lpr):
    """the SDDMM's dot of the rows of q with the rows of k (both (E, n), one dtype) on a group of lpr lanes, in the dtype"""
    dt = q.dtype
    E, n = q.shape
    w = 16 // dt.itemsize
    j = np.arange(n)
    lane = (j // w) % lpr
    step = (j // w) // lpr * w + j % w                  # position of column j in its lane's chain
    nstep = int(step.max()) + 1 if n else 0
    qa = np.zeros((E, nstep, lpr), dt)
    ka = np.zeros((E, nstep, lpr), dt)
    qa[:, step, lane] = q
    ka[:, step, lane] = k
    acc = np.zeros((E, lpr), dt)
    for t in range(nstep):
        acc = SR.fma(qa[:, t, :], ka[:, t, :], acc)
    lanes = np.arange(lpr)
    s = 1
    while s < lpr:
        acc = acc + acc[:, lanes ^ s]
        s *= 2
    return acc[:, 0]


def scores_replay(rp, ci, Q, K, scale, bias=None, lpr=None, chunk=2048):
    """the kernel's scores per nonzero, in the dtype: dot * scale (+ bias); lpr None: the SDDMM's own group for nk"""
    dt = Q.dtype
    rows = rows_of(rp)
    lpr = group_of(Q.shape[1], dt) if lpr is None else lpr
    dots = np.empty(ci.size, dt)
    for a in range(0, ci.size, chunk):
        dots[a:a + chunk] = dots_replay(Q[rows[a:a + chunk]], K[ci[a:a + chunk]], lpr)
    s = dots * dt.type(scale)
    if bias is not None:
        s = s + bias.astype(dt)
    return s.astype(dt), dots


def replay(rp, ci, Q, K, V, scale, bias=None, exp=np.exp):
    """(O, lse, p) in the operands' dtype, in the kernel's order"""
    dt = Q.dtype
    nrow, nv = rp.size - 1, V.shape[1]
    s, _ = scores_replay(rp, ci, Q, K, scale, bias, lpr_of(Q.shape[1], nv, dt))
    lens = np.diff(rp).astype(np.int64)
    O = np.zeros((nrow, nv), dt)
    lse = np.full(nrow, -np.inf, dt)
    p = np.zeros(ci.size, dt)
    nb_of = (lens + UNR - 1) // UNR
    ninf = dt.type(-np.inf)
    for nb in np.unique(nb_of[nb_of > 0]):
        r = np.flatnonzero(nb_of == nb)
        pos = np.arange(nb * UNR, dtype=np.int64)[None, :]
        valid = pos < lens[r][:, None]
        idx = rp[r].astype(np.int64)[:, None] + np.minimum(pos, lens[r][:, None] - 1)
        S = np.where(valid, s[idx], ninf).astype(dt)
        m = np.full(r.size, ninf, dt)
        l = np.zeros(r.size, dt)
        acc = np.zeros((r.size, nv), dt)
        with np.errstate(invalid="ignore", over="ignore"):
            for b in range(nb):
                Sb = S[:, b * UNR:(b + 1) * UNR]
                mn = np.maximum(m, Sb.max(axis=1))
                live = mn != ninf
                safe = np.where(live, mn, 0).astype(dt)
                f = np.where(live, np.asarray(exp((m - safe).astype(dt))), 1).astype(dt)
                e = np.where(live[:, None], np.asarray(exp((Sb - safe[:, None]).astype(dt))), 0).astype(dt)
                m = mn
                l = l * f
                for u in range(UNR):
                    l = l + e[:, u]
                acc = acc * f[:, None]
                for u in range(UNR):
                    on = e[:, u] != 0                   # (a masked or padded slot adds exactly nothing)
                    if on.any():
                        acc[on] = SR.fma(np.broadcast_to(e[on, u, None], (int(on.sum()), nv)), V[ci[idx[on, b * UNR + u]]], acc[on])
            masked = m == ninf
            lsafe = np.where(masked, 1, l).astype(dt)
            O[r] = np.where(masked[:, None], 0, acc / lsafe[:, None])
            lse[r] = np.where(masked, ninf, m + np.log(lsafe))
            msafe = np.where(masked, 0, m).astype(dt)
            pr = np.where(masked[:, None], 0, np.asarray(exp((S - msafe[:, None]).astype(dt))) / lsafe[:, None]).astype(dt)
        p[idx[valid]] = pr[valid]
    return O, lse, p


# ---- test data --------------------------------------------------------------------------------------------------------

SPECIAL_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 200, 5000, 0, 2, 4, 16, 32)
NROW, NCOL = 256, 5200
WIDTHS = ((1, 1), (3, 3), (16, 16), (17, 17), (33, 33), (64, 64), (65, 65), (129, 129), (257, 257), (520, 520), (8, 40), (130, 4),
          (32, 32), (128, 128), (256, 256), (512, 520), (4, 1030), (1030, 8))
WIDTHS_F32_EXTRA = ((8, 2100),)          # past one V block of the fp32 kernel (8 pieces of 64 lanes: 2048 columns)


@functools.lru_cache(maxsize=None)
def matrix(seed=11):
    """(rp, ci): NROW rows over NCOL columns; the first rows have SPECIAL_LENGTHS, the others 0 .. 40 entries"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, NROW)
    lens[:len(SPECIAL_LENGTHS)] = SPECIAL_LENGTHS
    cols = [np.sort(rng.choice(NCOL, size=int(n), replace=False)) for n in lens]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci


def operands(nk, nv, dtype, seed, nrow=NROW, ncol=NCOL):
    """Q, K, V in the dtype (standard normal) and the scale 1 / sqrt(nk): scores of unit variance, T well inside the data rule"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nrow, nk)).astype(dt)
    K = rng.standard_normal((ncol, nk)).astype(dt)
    V = rng.standard_normal((ncol, nv)).astype(dt)
    return Q, K, V, float(dt.type(1.0 / np.sqrt(nk)))


@functools.lru_cache(maxsize=None)
def case(nk, nv, dtype):
    """(rp, ci, Q, K, V, scale, ref) of one parity case, computed once and read-only"""
    dt = np.dtype(dtype)
    rp, ci = matrix()
    Q, K, V, scale = operands(nk, nv, dt, 100 * nk + nv + (dt == np.float32))
    ref = reference(rp, ci, Q, K, V, scale)
    assert ref["T"].max() <= SR.T_MAX[dt]
    for a in (Q, K, V):
        a.setflags(write=False)
    return rp, ci, Q, K, V, scale, ref


def parity_cases():
    for dtype in ("float64", "float32"):
        for nk, nv in WIDTHS + (WIDTHS_F32_EXTRA if dtype == "float32" else ()):
            yield nk, nv, dtype


STEEP_LENGTHS = (8, 9, 16, 17, 24, 40, 59, 60, 61, 64)


@functools.lru_cache(maxsize=None)
def steep_case(dtype, nk=24, nv=20):
    """Rows whose scores are led by a bias: for every length of STEEP_LENGTHS one row that ascends by 0.9 per entry (every batch
    raises the maximum), one that descends by 0.9 (none after the first does), one whose maximum, 50 above the rest, is the
    row's last entry (in the last partial batch where the length is no multiple of 8) and one with every second entry masked.
    T <= 60: inside the data rule of both dtypes.  Returns (rp, ci, bias, Q, K, V, scale, ref)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(5)
    lens, bias = [], []
    for n in STEEP_LENGTHS:
        ramp = 0.9 * np.arange(n)
        last = np.zeros(n)
        last[-1] = 50.0
        half = np.where(np.arange(n) % 2 == 1, -np.inf, 0.25 * np.arange(n))
        for b in (ramp, -ramp, last, half):
            lens.append(n)
            bias.append(b)
    lens = np.array(lens)
    ncol = 80
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(ncol, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    bias = np.concatenate(bias)
    Q, K, V, scale = operands(nk, nv, dt, 77, nrow=lens.size, ncol=ncol)
    scale = float(dt.type(0.05))
    ref = reference(rp, ci, Q, K, V, scale, bias.astype(dt))
    assert 40 < ref["T"].max() <= 60
    return rp, ci, bias, Q, K, V, scale, ref


worst = SR.worst
