"""Reference, error bound, CPU replay and test data of the fused GAT attention over a CSR pattern (csrc/gat_kernels.hip):

    z = el[i, h] + er[c_p, h],   a = z > 0 ? z : slope z,   s = a (+ val_p),   O[i]_h = sum_p softmax_p(s) V[c_p]_h

and of its backward: p = exp(s - lse), dP = <dO[i]_h, V[c]_h>, D = <dO[i]_h, O[i]_h>, dS = p (dP - D), dZ = dS g with
g = z > 0 ? 1 : slope;  d_el[i, h] = sum_row dZ,  d_er[c, h] = sum_column dZ,  dV[c]_h = sum_column p dO[i]_h.

From the scores on the kernels ARE the fused attention's (csrc/attention_kernels.hip, attention_bwd_kernels.hip), so everything
here is attention_ref / attention_bwd_ref on a zero dot (Q = K = 0, one column) with the score as the bias; what is this
file's own is the score, its error D, and the two scalar sums of the backward.

Bound (derived in DESIGN.md 5o, not measured; u = 2^-53 / 2^-24; the reference is np.longdouble on the dtype-rounded el, er, V,
dO, values and slope).  The sign of fl(el + er) is the sign of el + er, so kernel and reference take the same branch, and

    D = max_p u (2 |a_p| + [bias] |s_p|)      z and slope z: (1 + u)^2 - 1 on |a|; the bias addition: u |s|

replaces 5j's D in c = (2 L + 4 T + 10 R + 9) u + 2 D; the bounds of O, p_out, lse (5j) and of delta, ds_out, dV (5l, with this c
and D) keep their form.  dZ = dS g is one more rounding of a number bounded by S_p |g_p|, and the sums are L (Lc) - 1 additions:

    |d_el - ref| <= 1.01 (e_S(i) + (L_i + 1) u) sum_row S_p |g_p|
    |d_er - ref| <= 1.01 sum_column (e_S(i_p) + (Lc + 1) u) S_p |g_p|

replay() repeats the kernels' FIXED ORDER in numpy: the three roundings of the score in the dtype, then attention_ref.replay and
attention_bwd_ref.replay on those scores, then dZ and its sequential sums.  numpy's exp is not the device library's, so the
replay shows that the ORDER meets the bound and does not predict the device's bits."""
import functools

import numpy as np

import attention_bwd_ref as B
import attention_ref as R
import softmax_ref as SR

U = SR.U
worst = SR.worst
W = {"float64": 2, "float32": 4}
FWD_KEYS = ("O", "lse", "p")
BWD_KEYS = ("delta", "ds", "d_el", "d_er", "dV")


def _zeros(n, dt):
    return np.zeros((n, 1), dt)


# ---- the scores -------------------------------------------------------------------------------------------------------

def scores_exact(rp, ci, el, er, slope, h, val=None):
    """(s, a, g) of head h per nonzero in np.longdouble from the dtype-rounded inputs (slope rounded to the dtype once)"""
    dt = el.dtype
    rows = R.rows_of(rp)
    sl = np.longdouble(dt.type(slope))
    with np.errstate(invalid="ignore"):
        z = el[rows, h].astype(np.longdouble) + er[ci, h].astype(np.longdouble)
        a = np.where(z > 0, z, sl * z)
        s = a if val is None else a + val.astype(dt).astype(np.longdouble)
    return s, a, np.where(z > 0, np.longdouble(1), sl)


def scores_dtype(rp, ci, el, er, slope, h, val=None):
    """(s, g) of head h per nonzero as the kernels form them: every step rounded to the dtype on its own"""
    dt = el.dtype
    rows = R.rows_of(rp)
    sl = dt.type(slope)
    with np.errstate(invalid="ignore"):
        z = (el[rows, h] + er[ci, h]).astype(dt)
        a = np.where(z > 0, z, (sl * z).astype(dt)).astype(dt)
        s = a if val is None else (a + val.astype(dt)).astype(dt)
    return s, np.where(z > 0, dt.type(1), sl).astype(dt)


# ---- the reference and the bound --------------------------------------------------------------------------------------

def reference(rp, ci, el, er, V, slope, val=None, dO=None):
    """name -> (np.longdouble reference, bound), each shaped as the kernels' output: O (rows, H dv), lse (rows, H), p (nnz, H) and,
    with dO, delta (rows, H), ds (nnz, H), d_el (rows, H), d_er (columns, H), dV (columns, H dv); also "T": the widest spread"""
    dt = V.dtype
    u = U[dt]
    nrow, ncol, nnz, H = rp.size - 1, V.shape[0], ci.size, el.shape[1]
    dv = V.shape[1] // H
    ld = np.longdouble
    out = {k: (np.zeros(s, ld), np.zeros(s, ld)) for k, s in (("O", (nrow, H * dv)), ("lse", (nrow, H)), ("p", (nnz, H)))}
    if dO is not None:
        out.update({k: (np.zeros(s, ld), np.zeros(s, ld)) for k, s in (("delta", (nrow, H)), ("ds", (nnz, H)), ("d_el", (nrow, H)),
                                                                          ("d_er", (ncol, H)), ("dV", (ncol, H * dv)))})
    T = 0.0
    lens = np.diff(rp)
    ne = np.flatnonzero(lens > 0)
    for h in range(H):
        sv = slice(h * dv, (h + 1) * dv)
        s, a, g = scores_exact(rp, ci, el, er, slope, h, val)
        with np.errstate(invalid="ignore"):
            derr = np.where(np.isfinite(s), 2 * np.abs(a) + (np.abs(s) if val is not None else 0), 0)
        if dO is None:
            fwd = R.reference(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), V[:, sv], 1.0, s)
        else:
            bw = B.reference(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), V[:, sv], dO[:, sv], 1.0, s, ncol=ncol)
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
        e_S = B.coeffs(bw, dt)[1]
        tm, cit, rpt = bw["tmap"], bw["cit"], bw["rpt"]
        Lc = np.diff(rpt).astype(np.float64)
        dz, Sg = bw["ds"] * g, bw["S"] * np.abs(g)
        d_el = B._seg_sum(dz[:, None], rp)[:, 0]
        d_er = B._seg_sum(dz[tm, None], rpt)[:, 0]
        b_el = 1.01 * (e_S + (fwd["L"] + 1) * u) * B._seg_sum(Sg[:, None], rp)[:, 0]
        b_er = 1.01 * B._seg_sum(((e_S[cit] + (Lc[R.rows_of(rpt)] + 1) * u) * Sg[tm])[:, None], rpt)[:, 0]
        for k, ref, bnd in (("delta", bw["delta"], B.bound_delta(bw, dt)), ("ds", bw["ds"], B.bound_ds(bw, dt)), ("d_el", d_el, b_el),
                            ("d_er", d_er, b_er), ("dV", bw["dV"], B.bound_dV(bw, dt))):
            sel = sv if k == "dV" else h
            out[k][0][:, sel], out[k][1][:, sel] = ref, bnd
    out["T"] = T
    return out


def ratios(got, ref):
    """worst |got - ref| / bound per output of `got` (name -> array); lse: -inf must match exactly and is left out of the ratio"""
    out = {}
    for k, v in got.items():
        want, bnd = ref[k]
        v = np.asarray(v).reshape(want.shape)
        if k == "lse":
            live = np.isfinite(want.astype(np.float64))
            assert np.array_equal(np.isfinite(v), live) and (v[~live] == -np.inf).all(), "lse of empty / masked rows"
            out[k] = worst(v[live], want[live], bnd[live])[0]
            continue
        assert np.isfinite(v).all(), (k, "non-finite output")
        out[k] = worst(v.ravel(), want.ravel(), bnd.ravel())[0]
    return out


# ---- the replay -------------------------------------------------------------------------------------------------------

def seq_sum(rp, x):
    """per row of rp, the sum of x's entries from +0 in ascending p, one addition in the dtype per entry"""
    return B._chain(rp, x, np.ones((1, 1), x.dtype), np.zeros(x.size, np.int64))[:, 0]


def replay(rp, ci, el, er, V, slope, val=None, dO=None, exp=np.exp):
    """name -> array in the operands' dtype, in the kernels' order (the keys of reference())"""
    dt = V.dtype
    nrow, ncol, nnz, H = rp.size - 1, V.shape[0], ci.size, el.shape[1]
    dv = V.shape[1] // H
    out = dict(O=np.zeros((nrow, H * dv), dt), lse=np.zeros((nrow, H), dt), p=np.zeros((nnz, H), dt))
    if dO is not None:
        out.update(delta=np.zeros((nrow, H), dt), ds=np.zeros((nnz, H), dt), d_el=np.zeros((nrow, H), dt), d_er=np.zeros((ncol, H), dt),
                   dV=np.zeros((ncol, H * dv), dt))
        rpt, cit, tmap = B.transpose(rp, ci, ncol)
    for h in range(H):
        sv = slice(h * dv, (h + 1) * dv)
        s, g = scores_dtype(rp, ci, el, er, slope, h, val)
        Vh = np.ascontiguousarray(V[:, sv])
        O, lse, p = R.replay(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), Vh, 1.0, s, exp=exp)
        out["O"][:, sv], out["lse"][:, h], out["p"][:, h] = O, lse, p
        if dO is None:
            continue
        bw = B.replay(rp, ci, _zeros(nrow, dt), _zeros(ncol, dt), Vh, O, lse, np.ascontiguousarray(dO[:, sv]), 1.0, s, exp=exp)
        dz = np.where(bw["ds"] == 0, 0, bw["ds"] * g).astype(dt)
        out["delta"][:, h], out["ds"][:, h], out["dV"][:, sv] = bw["delta"], bw["ds"], bw["dV"]
        out["d_el"][:, h], out["d_er"][:, h] = seq_sum(rp, dz), seq_sum(rpt, dz[tmap])
    return out


# ---- test data --------------------------------------------------------------------------------------------------------

SPECIAL_LENGTHS = (0, 1, 7, 8, 9, 17, 70, 0, 2, 16)
NROW, NCOL, K0 = 40, 80, 50              # K0: the rows of the first source of the two-source codes
EMPTY_COL = 79


@functools.lru_cache(maxsize=None)
def matrix(seed=3):
    """(rp, ci): NROW rows over NCOL columns; the first rows have SPECIAL_LENGTHS -- the one of 70 entries passes a chunk of 64
    lanes -- the others 0 .. 12 entries; no row names EMPTY_COL; both sides of K0 are named"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 13, NROW)
    lens[:len(SPECIAL_LENGTHS)] = SPECIAL_LENGTHS
    cols = [np.sort(rng.choice(NCOL - 1, size=int(n), replace=False)) for n in lens]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    assert (ci < K0).any() and (ci >= K0).any() and not (ci == EMPTY_COL).any()
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci


def two_source_codes(ci, k0=K0):
    """the codes of a two-source handle: the columns below k0 as they are, column c >= k0 as ~(c - k0)"""
    return np.where(ci < k0, ci, ~(ci - k0)).astype(np.int32)


# The chunk pattern: every length at which a kernel that walks a row (or a column of A) in chunks of LPR = 8, 16, 32 or 64 entries
# takes another trip, on both sides
CHUNK_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 200)      # of the first rows; the last row is empty too
CHUNK_NROW, CHUNK_NCOL, CHUNK_K0 = 280, 256, 128
CHUNK_HUB, CHUNK_EMPTY_COL = 5, 17
CHUNK_COLS = {1: 18, 8: 19, 9: 20, 63: 130, 64: 131, 65: 132}        # length -> the column of exactly that many entries
CHUNK_SHUFFLED = 65                      # rows from this length on hold their columns in a shuffled order


@functools.lru_cache(maxsize=None)
def chunk_matrix(seed=23):
    """(rp, ci): CHUNK_NROW rows over CHUNK_NCOL columns.  The first rows have CHUNK_LENGTHS, the last one is empty, the others
    2 .. 6 entries; every row of two or more entries names CHUNK_HUB (more than four chunks of 64 on the column side); no row names
    CHUNK_EMPTY_COL and the columns of CHUNK_COLS have exactly 1, 8, 9, 63, 64 and 65 entries, from consecutive short rows; the
    rows of CHUNK_SHUFFLED entries and more are not in ascending column order; both sides of CHUNK_K0 are named by the long rows"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 7, CHUNK_NROW)
    lens[:len(CHUNK_LENGTHS)] = CHUNK_LENGTHS
    lens[-1] = 0
    extra = np.full(CHUNK_NROW, -1)
    r = 20
    for n in sorted(CHUNK_COLS):
        extra[r:r + n] = CHUNK_COLS[n]
        r += n
    assert r < CHUNK_NROW - 1
    pool = np.setdiff1d(np.arange(CHUNK_NCOL), [CHUNK_HUB, CHUNK_EMPTY_COL] + list(CHUNK_COLS.values()))
    cols = []
    for r, n in enumerate(lens):
        n = int(n)
        if n < 2:
            cols.append(rng.choice(pool, size=n, replace=False))
            continue
        own = [CHUNK_HUB] + ([extra[r]] if extra[r] >= 0 else [])
        c = np.sort(np.concatenate([own, rng.choice(pool, size=n - len(own), replace=False)]))
        cols.append(rng.permutation(c) if n >= CHUNK_SHUFFLED else c)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci


def check_chunk_matrix():
    """the properties the chunk tests rely on"""
    rp, ci = chunk_matrix()
    lens, cnt = np.diff(rp), np.bincount(ci, minlength=CHUNK_NCOL)
    nspec = len(CHUNK_LENGTHS)
    assert rp.size - 1 == CHUNK_NROW and cnt.size == CHUNK_NCOL and 1500 <= ci.size <= 3000, (rp.size, cnt.size, ci.size)
    assert tuple(lens[:nspec]) == CHUNK_LENGTHS and lens[-1] == 0 and (lens == 0).sum() == 2
    assert lens[nspec:-1].min() >= 2 and lens[nspec:-1].max() <= 6
    assert {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 200} <= set(lens.tolist())
    for i in range(CHUNK_NROW):
        c = ci[rp[i]:rp[i + 1]]
        assert np.unique(c).size == c.size, "a row names a column once"
        assert (lens[i] >= 2) == bool((c == CHUNK_HUB).any()), "every row of two or more entries names the hub, no other"
        if lens[i] >= CHUNK_SHUFFLED:
            assert (np.diff(c) < 0).any(), (i, "in ascending order")
            assert (c < CHUNK_K0).any() and (c >= CHUNK_K0).any(), (i, "names one source only")
    assert cnt[CHUNK_HUB] == (lens >= 2).sum() > 4 * 64 + 8 and cnt[CHUNK_EMPTY_COL] == 0
    for n, c in CHUNK_COLS.items():
        assert cnt[c] == n, (c, cnt[c], n)
    codes = two_source_codes(ci, CHUNK_K0)
    assert (codes < 0).any() and (codes >= 0).any() and (~codes[codes < 0]).max() < CHUNK_NCOL - CHUNK_K0


def operands(dtype, H, dv, spread, seed, nrow=NROW, ncol=NCOL):
    """el, er, V, dO in the dtype: standard normal, el and er times `spread` (the scale of the scores)"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    el = (spread * rng.standard_normal((nrow, H))).astype(dt)
    er = (spread * rng.standard_normal((ncol, H))).astype(dt)
    V = rng.standard_normal((ncol, H * dv)).astype(dt)
    dO = rng.standard_normal((nrow, H * dv)).astype(dt)
    return el, er, V, dO


def widths(dtype):
    """one head's widths: 1, 5, the last of the group of 8 lanes and the first past it, one past 32 W (64 lanes) and past 64 W (two
    pieces per lane)"""
    w = W[np.dtype(dtype).name]
    return (1, 5, 8 * w, 8 * w + 1, 32 * w + w, 64 * w + w)


def second_block_width(dtype):
    """the forward's second V block: past 8 pieces of 64 lanes"""
    w = W[np.dtype(dtype).name]
    return 8 * 64 * w + w


# The kernel instance (LPR lanes per unit, P pieces per lane) comes from (dtype, nv) alone, with W = 16 / sizeof(T).  gat_fwd in
# csrc/gat_kernels.hip:
#     if (a.nv <= 8 * W)   return launch_gat<T, 8, 1>(a, s);
#     if (a.nv <= 16 * W)  return launch_gat<T, 16, 1>(a, s);
#     if (a.nv <= 32 * W)  return launch_gat<T, 32, 1>(a, s);
#     if (a.nv <= 64 * W)  return launch_gat<T, 64, 1>(a, s);
#     if (a.nv <= 128 * W) return launch_gat<T, 64, 2>(a, s);
#     if (a.nv <= 256 * W) return launch_gat<T, 64, 4>(a, s);
#     return launch_gat<T, 64, 8>(a, s);
# gat_bwd there and gatv2_any in csrc/gatv2_kernels.hip (launch_gatv2) refuse nv > CAP = 256 W, have the same first five lines and end in
#     return launch_gat<T, 64, 4>(a, s);
KINDS = ("gat_fwd", "gat_bwd", "gatv2")
INSTANCES = ((8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (256, (64, 4)))    # (the last width in W, (LPR, P))
FWD_BLOCK = 512                          # in W: the forward's V block of 8 pieces of 64 lanes


def instance_of(kind, dtype, dv):
    """(LPR, P) of the kernel that serves one head's width dv; kind: one of KINDS"""
    assert kind in KINDS and dv >= 1
    w = W[np.dtype(dtype).name]
    for top, inst in INSTANCES:
        if dv <= top * w:
            return inst
    assert kind == "gat_fwd", (kind, dv, "is over the cap")
    return 64, 8


def chunk_widths(dtype, kind="gat_bwd"):
    """one head's widths on the chunk pattern: both sides of the thresholds 16 W, 32 W, 64 W and 128 W (8 W is in widths()), the cap
    256 W (P = 4, full), and one width that is no multiple of W strictly inside the 32-lane and the 64-lane range -- with the + 1
    widths these are the element path; for the forward of GAT also the first width of P = 8 and its one V block, full"""
    w = W[np.dtype(dtype).name]
    out = (16 * w, 16 * w + 1, 17 * w + 1, 32 * w, 32 * w + 1, 40 * w + 1, 64 * w, 64 * w + 1, 128 * w, 128 * w + 1, 256 * w)
    return out + ((256 * w + 1, FWD_BLOCK * w) if kind == "gat_fwd" else ())


SPREADS = (0.5, 6.0)
SLOPE = 0.2


def bound_cases():
    """(dtype, H, dv, spread): what test_gpu_gat.py holds against the bound and test_gat_ref.py replays"""
    for dtype in ("float64", "float32"):
        for i, dv in enumerate(widths(dtype)):
            for H in (1, 3):
                yield dtype, H, dv, SPREADS[(i + H) % 2]


@functools.lru_cache(maxsize=None)
def case(dtype, H, dv, spread):
    """(rp, ci, el, er, V, dO, ref) of one bound case on matrix(), computed once and read-only"""
    dt = np.dtype(dtype)
    rp, ci = matrix()
    el, er, V, dO = operands(dt, H, dv, spread, 1000 * H + dv + (dt == np.float32))
    ref = reference(rp, ci, el, er, V, SLOPE, None, dO)
    assert ref["T"] <= SR.T_MAX[dt], ref["T"]
    for x in (el, er, V, dO):
        x.setflags(write=False)
    return rp, ci, el, er, V, dO, ref


def chunk_bound_cases():
    """(dtype, H, dv, spread, backward) on chunk_matrix(): what the chunk tests hold against the bound on the GPU and replay on the
    CPU.  H = 3 and H = 1 on the widths up to 64 W + 1, H = 1 above (the reference's cost grows with H dv); the widths past the cap
    are the forward's alone"""
    for dtype in ("float64", "float32"):
        w = W[dtype]
        for i, dv in enumerate(chunk_widths(dtype, "gat_fwd")):
            for H in ((1, 3) if dv <= 64 * w + 1 else (1,)):
                yield dtype, H, dv, SPREADS[(i + H) % 2], dv <= 256 * w


@functools.lru_cache(maxsize=None)
def chunk_case(dtype, H, dv, spread, backward=True):
    """(rp, ci, el, er, V, dO, ref) of one bound case on chunk_matrix(), computed once and read-only (forward only: dO is None)"""
    dt = np.dtype(dtype)
    rp, ci = chunk_matrix()
    el, er, V, dO = operands(dt, H, dv, spread, 3000 * H + dv + (dt == np.float32), nrow=CHUNK_NROW, ncol=CHUNK_NCOL)
    dO = dO if backward else None
    ref = reference(rp, ci, el, er, V, SLOPE, None, dO)
    for x in (el, er, V, dO):
        if x is not None:
            x.setflags(write=False)
    return rp, ci, el, er, V, dO, ref


@functools.lru_cache(maxsize=None)
def second_block_case(dtype):
    """12 rows of matrix() at second_block_width, one head, forward only: (rp, ci, el, er, V, ref)"""
    dt = np.dtype(dtype)
    rp, ci = matrix()
    nrow = 12
    rp, ci = rp[:nrow + 1], ci[:int(rp[nrow])]
    el, er, V, _ = operands(dt, 1, second_block_width(dt), 1.0, 77, nrow=nrow)
    return rp, ci, el, er, V, reference(rp, ci, el, er, V, SLOPE)


@functools.lru_cache(maxsize=None)
def steep_case(dtype, H=3, dv=20):
    """attention_ref.steep_case's rows -- ascending, descending, late-peak and half-masked, T up to 60 -- with its bias as the
    matrix's values (bias = 1) under small el and er: (rp, ci, val, el, er, V, dO, ref); 80 columns"""
    dt = np.dtype(dtype)
    rp, ci, val = R.steep_case(dtype)[:3]
    el, er, V, dO = operands(dt, H, dv, 0.25, 91, nrow=rp.size - 1, ncol=80)
    ref = reference(rp, ci, el, er, V, SLOPE, val, dO)
    assert 40 < ref["T"] <= SR.T_MAX[dt], ref["T"]
    return rp, ci, val, el, er, V, dO, ref
