"""Reference, error bounds, CPU replay and test data of the row softmax over a CSR pattern (csrc/softmax_kernels.hip).

Definition, per row r with entries p in [rp[r], rp[r + 1]):  m = max s,  e = exp(s - m),  y = e / sum e;  backward
D = sum y dy,  ds = y (dy - D).  An entry of -inf is a masked edge (y exactly 0); a row of -inf only gives zeros.

Bounds (derived, not measured; u = 2^-53 / 2^-24, L the row's length, T = max (m - s) over the row's finite entries; the
reference is np.longdouble on the dtype-rounded inputs):

    forward    |y - ref|  <= 1.01 (L + 2 T + 8) u ref
        the subtraction's rounding moves an exponent by at most T u, in the numerator and in the terms of the sum: 2 T u;
        exp within E ulp in both, E = 2 allowed: 4 E u = 8 u, the division's rounding inside; a sum of L positive terms in
        any order errs by (L - 1) u.
    backward   |ds - ref| <= 1.01 u |y_p| ((L + 2) S + 2 |dy_p|),  S = sum_q |y_q dy_q|
        an L-term FMA dot errs by at most L u S in any order; the subtraction dy - D adds u (|dy| + |D|) <= u (|dy| + S), the
        product one more rounding of |y| (|dy| + S).

Data rule: no result near the subnormal range; T <= 60 (fp32) and <= 600 (fp64), -inf entries aside.

replay_fwd / replay_bwd repeat the kernel's FIXED ORDER in numpy: 64 strided partials per row (partial k adds entries k,
k + 64, ... in ascending order from +0), then the balanced binary tree over k (k ^ 1, k ^ 2, ... k ^ 32).  numpy has no FMA:
the backward's is emulated with one rounding (fma: fp32 exactly, through the exact fp64 product and a tie correction; fp64 by
an error-free product and sum, whose one approximation shows in about one operation in 2^50), so replay_bwd gives the bits of
any IEEE device for the same y and dy.  numpy's exp is not the device's: with it replay_fwd shows that the ORDER meets the
bounds and does not predict the device's bits; given the device library's exp (its `exp` argument) it does."""
import functools

import numpy as np

U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
T_MAX = {np.dtype(np.float64): 600.0, np.dtype(np.float32): 60.0}
SPREADS = (1, 8, "max")
_LANE = np.arange(64)


def rows_of(rp):
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def _seg(rp):
    """start offsets of the non-empty rows (np.ufunc.reduceat over them reduces exactly the rows) and their row numbers"""
    lens = np.diff(rp)
    ne = np.flatnonzero(lens > 0)
    return (rp[ne] - rp[0]).astype(np.intp), ne


def _view(rp, a):
    return a[rp[0]:rp[-1]]


def reference_fwd(rp, s):
    """(ref, L, T) per entry of the rows, np.longdouble / float: the exact softmax of the dtype-rounded scores"""
    x = _view(rp, s).astype(np.longdouble)
    nrow = rp.size - 1
    starts, ne = _seg(rp)
    rows = rows_of(rp)
    m = np.full(nrow, -np.inf, np.longdouble)
    if ne.size:
        m[ne] = np.maximum.reduceat(x, starts)
    with np.errstate(invalid="ignore"):
        d = m[rows] - x
        e = np.where(np.isfinite(d), np.exp(-np.where(np.isfinite(d), d, 0)), 0).astype(np.longdouble)
    tot = np.zeros(nrow, np.longdouble)
    if ne.size:
        tot[ne] = np.add.reduceat(e, starts)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = np.where(tot[rows] > 0, e / tot[rows], 0)
    T = np.zeros(nrow)
    if ne.size:
        T[ne] = np.maximum.reduceat(np.where(np.isfinite(d), d, 0).astype(np.float64), starts)
    return ref, np.diff(rp)[rows].astype(np.float64), T[rows]


def bound_fwd(ref, L, T, dtype):
    return 1.01 * (L + 2 * T + 8) * U[np.dtype(dtype)] * ref


def reference_bwd(rp, y, dy):
    """(ref, L, S) per entry: ds in np.longdouble from the dtype-rounded y and dy, and S = the row's sum of |y dy|"""
    yl, gl = _view(rp, y).astype(np.longdouble), _view(rp, dy).astype(np.longdouble)
    nrow = rp.size - 1
    starts, ne = _seg(rp)
    rows = rows_of(rp)
    D, S = np.zeros(nrow, np.longdouble), np.zeros(nrow, np.longdouble)
    if ne.size:
        D[ne] = np.add.reduceat(yl * gl, starts)
        S[ne] = np.add.reduceat(np.abs(yl * gl), starts)
    return yl * (gl - D[rows]), np.diff(rp)[rows].astype(np.float64), S[rows]


def bound_bwd(y, dy, L, S, dtype):
    yl, gl = np.abs(y.astype(np.longdouble)), np.abs(dy.astype(np.longdouble))
    return 1.01 * U[np.dtype(dtype)] * yl * ((L + 2) * S + 2 * gl)


def _two_sum(a, b):
    """(s, e): s = fl(a + b) and a + b = s + e exactly"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c):
    """fl(a * b + c) with ONE rounding, elementwise, for float32 or float64 arrays of one dtype (no overflow, no subnormal
    product).  float32: the product is exact in float64 and so is the sum but for one rounding to 53 bits; where that lands
    exactly half way between two float32 numbers the sign of its error decides, as it would have for the exact sum.  float64:
    Dekker's error-free product ph + pl and Knuth's error-free sum s + e of ph and c; the result is fl(s + fl(e + pl))."""
    a, b, c = np.broadcast_arrays(np.asarray(a), np.asarray(b), np.asarray(c))
    dt = a.dtype
    assert dt == b.dtype == c.dtype and dt in U, (a.dtype, b.dtype, c.dtype)
    if dt == np.float32:
        p = a.astype(np.float64) * b.astype(np.float64)
        s, e = _two_sum(p, c.astype(np.float64))
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)
        up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
        with np.errstate(invalid="ignore", over="ignore"):
            go_up = (d > 0) & (2 * d == up.astype(np.float64) - r) & (e > 0)
            go_dn = (d < 0) & (-2 * d == r.astype(np.float64) - dn) & (e < 0)
        return np.where(go_up, up, np.where(go_dn, dn, r))
    split = 134217729.0                                     # 2^27 + 1
    ph = a * b
    t = a * split
    ah = t - (t - a)
    t = b * split
    bh = t - (t - b)
    al, bl = a - ah, b - bh
    pl = ((ah * bh - ph) + ah * bl + al * bh) + al * bl
    s, e = _two_sum(ph, c)
    return s + (e + pl)


def _fixed_order_sums(rp, a, b=None):
    """per row, the sum of a (b None) or of a * b with FMAs, in the kernel's order; a, b are views of the rows' entries"""
    dt = a.dtype
    lens = np.diff(rp).astype(np.int64)
    off = (rp[:-1] - rp[0]).astype(np.int64)
    out = np.zeros(lens.size, dt)
    nch = (lens + 63) // 64
    for c in np.unique(nch[nch > 0]):
        rows = np.flatnonzero(nch == c)
        pos = np.arange(c * 64, dtype=np.int64)[None, :]
        valid = pos < lens[rows][:, None]
        idx = np.where(valid, off[rows][:, None] + pos, 0)
        A = np.where(valid, a[idx], 0).astype(dt).reshape(rows.size, c, 64)
        B = None if b is None else np.where(valid, b[idx], 0).astype(dt).reshape(rows.size, c, 64)
        acc = np.zeros((rows.size, 64), dt)
        for k in range(c):
            if B is None:
                acc = acc + A[:, k, :]
            else:
                acc = fma(A[:, k, :], B[:, k, :], acc)
        for step in (1, 2, 4, 8, 16, 32):
            acc = acc + acc[:, _LANE ^ step]
        out[rows] = acc[:, 0]
    return out


def replay_fwd(rp, s, exp=np.exp):
    """the rows' softmax in the dtype of s, in the kernel's order (an array of rp[-1] - rp[0] entries).  exp: the exponential,
    on an array of the dtype holding 0, negative numbers and -inf; numpy's by default, which is not the device library's in
    the last bit -- a GPU test that wants the device's bits passes an exp evaluated by that library (outside the code under
    test), and the subtraction, the order of the sum and the division stay this function's"""
    x = _view(rp, s)
    dt = x.dtype
    nrow = rp.size - 1
    starts, ne = _seg(rp)
    rows = rows_of(rp)
    m = np.full(nrow, -np.inf, dt)
    if ne.size:
        m[ne] = np.maximum.reduceat(x, starts)
    live = np.isfinite(m)[rows]
    with np.errstate(invalid="ignore"):
        e = np.where(live, np.asarray(exp(np.where(live, x - m[rows], 0).astype(dt))), 0).astype(dt)
    tot = _fixed_order_sums(rp, e)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(live, e / tot[rows], 0).astype(dt)


def replay_bwd(rp, y, dy):
    yv, gv = _view(rp, y), _view(rp, dy)
    D = _fixed_order_sums(rp, yv, gv)
    return (yv * (gv - D[rows_of(rp)])).astype(yv.dtype)


# ---- test data ------------------------------------------------------------------------------------------------------

def scores(rp, dtype, spread, seed, masked=True):
    """Scores for the rows of rp (rp[0] == 0): uniform over a width of `spread` (1, 8 or "max" = the data rule's T) below a
    per-row offset, every row's extremes present from 2 finite entries on, and -- masked -- one -inf entry per row of 2+"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    lens = np.diff(rp)
    rows = rows_of(rp)
    width = (T_MAX[dt] - 0.5) if spread == "max" else float(spread)
    s = -width * rng.random(rows.size)
    first = rp[:-1][lens > 0]
    s[first] = 0.0
    s[first[lens[lens > 0] > 2] + 1] = -width          # the full spread, with room left for the masked entry
    s = (s + rng.uniform(-3, 3, lens.size)[rows]).astype(dt)
    if masked:
        r2 = np.flatnonzero(lens >= 2)
        s[rp[r2] + rng.integers(0, 1 << 30, r2.size) % lens[r2]] = -np.inf
    _ref, _L, T = reference_fwd(rp, s)
    assert T.size == 0 or T.max() <= T_MAX[dt], (T.max(), T_MAX[dt])
    return s


def grads(nnz, dtype, seed):
    return np.random.default_rng(seed).standard_normal(nnz).astype(dtype)


def long_row_lengths(seed=2):
    """tests/test_gpu_sddmm.py::_long_row_matrix's row lengths: 300 rows of 0 .. 5 entries around one of 70 000"""
    lens = np.random.default_rng(seed).integers(0, 6, 301)
    lens[150] = 70000
    return lens


# lengths either side of every multiple of 64 up to 192 (0 .. 200), of the register budgets of the four lane groups (8 LPR =
# 64, 128, 256, 512) and of longer chunk counts
SYNTH_LENGTHS = tuple(range(201)) + (255, 256, 257, 511, 512, 513, 4095, 4096, 4097)
# the kernel picks the lane group from nnz <= 12 / 24 / 48 nrow: row pointers whose mean sits AT and just OVER each threshold
LPR_EDGES = ((12, False, 8), (12, True, 16), (24, False, 16), (24, True, 32), (48, False, 32), (48, True, 64))


def rowptr_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def with_mean(lens, k, over):
    """lens followed by filler rows of one entry and a last one sized so that nnz == k * nrow exactly (over: one entry more)"""
    lens = list(lens)
    nnz, nrow = sum(lens), len(lens)
    fill = max(0, -(-(nnz - k * nrow) // (k - 1)))
    nnz, nrow = nnz + fill, nrow + fill
    last = k * (nrow + 1) - nnz
    assert last >= 1
    out = np.array(lens + [1] * fill + [last + (1 if over else 0)], dtype=np.int64)
    assert (out.sum() == k * out.size) != over and out.sum() <= k * out.size + 1
    return out


def lpr_of(rp):
    """the lane group the kernel picks for this row pointer (csrc/softmax_kernels.hip, sm_pick_lpr)"""
    nnz, nrow = int(rp[-1]) - int(rp[0]), rp.size - 1
    return 8 if nnz <= 12 * nrow else 16 if nnz <= 24 * nrow else 32 if nnz <= 48 * nrow else 64


@functools.lru_cache(maxsize=None)
def pattern(name):
    """the row pointers of the parity tests, by name"""
    from crp_spmm_amd import gen
    if name == "kkt3d(10)":
        return gen.kkt3d(10)[0].astype(np.int32)
    if name == "fem3d(7)":
        return gen.fem3d(7)[0].astype(np.int32)
    if name == "random_csr":
        return gen.random_csr(3000, 1700, 40, empty_every=13)[0].astype(np.int32)
    if name == "long_row":
        return rowptr_of(long_row_lengths())
    if name == "synthetic":
        return rowptr_of(SYNTH_LENGTHS)
    k, over = name.split(":")[1:]
    return rowptr_of(with_mean(SYNTH_LENGTHS, int(k), over == "over"))


PATTERNS = ("kkt3d(10)", "fem3d(7)", "random_csr", "long_row", "synthetic")
EDGE_PATTERNS = tuple("edge:%d:%s" % (k, "over" if over else "at") for k, over, _ in LPR_EDGES)


def parity_cases():
    """(pattern name, spread): the issue's matrices and the synthetic row pointer at every spread; the row pointers either
    side of the lane-group thresholds at the widest spread"""
    for name in PATTERNS:
        for spread in SPREADS:
            yield name, spread
    for name in EDGE_PATTERNS:
        yield name, "max"


@functools.lru_cache(maxsize=None)
def case(name, spread, dtype):
    """(rp, s, ref, bound, y, dy, ref_bwd, bound_bwd) of one parity case, computed once: y is the replay's forward result in
    `dtype` -- the y the backward under test reads"""
    dt = np.dtype(dtype)
    rp = pattern(name)
    seed = (sum(map(ord, name)) * 7 + SPREADS.index(spread)) * 2 + (dt == np.float32)
    s = scores(rp, dt, spread, seed)
    ref, L, T = reference_fwd(rp, s)
    y = replay_fwd(rp, s)
    dy = grads(s.size, dt, seed + 100000)
    rb, Lb, S = reference_bwd(rp, y, dy)
    out = (rp, s, ref, bound_fwd(ref, L, T, dt), y, dy, rb, bound_bwd(y, dy, Lb, S, dt))
    for a in out:
        a.setflags(write=False)
    return out


def worst(got, ref, bound):
    """max |got - ref| / bound (0 / 0 = 0, x / 0 = inf) and where"""
    err = np.abs(np.asarray(got).astype(np.longdouble) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    if ratio.size == 0:
        return 0.0, -1
    at = int(np.argmax(ratio))
    return float(ratio[at]), at
