"""fp64 references for the fp64 SpMM kernels (helper module of the tests; not a conftest).

exact_problem    data on which EVERY summation order, with or without FMA, gives the same bits: C must equal C_exact (np.array_equal)
f64_bound /
check_f64_bound  the entrywise error bound every summation order of an fp64 product meets on ordinary rounded data, against np.longdouble
rounded_problem  that rounded data: rows of A and rows of B on scales spread over 24 and 12 decades

Why not one relative Frobenius number: an error below 1e-12 ||C||_F in one entry passes it, and on matrices whose rows differ in scale
about half the entries of C lie below 1e-12 x the RMS entry (tests/test_fp64_ref.py prints the share).

The exact data.  A = D_r A0 D_c and B = D_c^-1 B0 with power-of-two diagonals D_r (row exponents uniform in [-40, 40]) and D_c (column
exponents uniform in [-30, 30]); A0 and B0 hold odd integers, the `wide` side below 2^27 and the other below 2^b,
b = 52 - 27 - ceil(log2(longest row)).  Then val[p] * B[c][j] = a0 b0 2^(row exponent) exactly, and in every row sum_p |a0 b0| < 2^53
(asserted): every partial sum of every subset of a row's products is an integer below 2^53 times 2^(row exponent) -- exact in fp64, fused
or not, in any order and any grouping.  An odd integer of up to 27 bits does not survive a trip through fp32 (24 bits), so running both
`wide` settings catches a value or a B element that leaks through a float.  A kernel whose value block holds a hole adds an exact 0:
signed zeros are not distinguished (np.array_equal: -0.0 == +0.0)."""
from collections import namedtuple

import numpy as np

from fp32_ref import split_two_source  # noqa: F401  (shared with the fp32 kernel tests)

assert np.finfo(np.longdouble).nmant >= 63, "the fp64 bound needs an extended-precision np.longdouble reference"

U64 = 2.0 ** -53          # unit roundoff of fp64
WIDE_BITS = 27
ROW_EXP, COL_EXP = 40, 30

Exact = namedtuple("Exact", "val B C_exact A0 B0 row_exp col_exp")


def _odd(rng, bits, size):
    """Odd integers of either sign below 2^bits in magnitude (int64)."""
    mag = 2 * rng.integers(0, 1 << (bits - 1), size=size, dtype=np.int64) + 1
    return np.where(rng.integers(0, 2, size=size) == 1, mag, -mag)


def exact_parts(rowptr, colidx, k, n, rng, wide, like=None):
    """exact_problem with its ingredients (Exact: val, B, C_exact, A0, B0 as int64, the row and column exponents).  like: an Exact of the
    same pattern, k and n -- a second value set for it: new integers A0, the same exponents and the same B."""
    import oracle
    assert wide in ("A", "B"), wide
    rp = np.asarray(rowptr, dtype=np.int64)
    ci = np.asarray(colidx, dtype=np.int64)
    m, nnz = rp.size - 1, int(rp[-1])
    assert nnz == 0 or (ci[:nnz].min() >= 0 and ci[:nnz].max() < k), "plain column indices (split two sources afterwards)"
    lens = np.diff(rp)
    longest = max(int(lens.max()) if m else 1, 1)
    narrow_bits = 52 - WIDE_BITS - int(np.ceil(np.log2(longest)))
    assert narrow_bits >= 2, ("rows too long for the exact budget", longest)
    bits_a, bits_b = (WIDE_BITS, narrow_bits) if wide == "A" else (narrow_bits, WIDE_BITS)
    A0 = _odd(rng, bits_a, nnz)
    if like is None:
        B0 = _odd(rng, bits_b, (k, n))
        row_exp = rng.integers(-ROW_EXP, ROW_EXP + 1, size=m)
        col_exp = rng.integers(-COL_EXP, COL_EXP + 1, size=k)
    else:
        B0, row_exp, col_exp = like.B0, like.row_exp, like.col_exp
        assert B0.shape == (k, n) and np.abs(B0).max() < (1 << bits_b)
    rows = np.repeat(np.arange(m), lens)
    # the budget: sum_p |a0 b0| < 2^53 for every entry of C (as integers: |A0| |B0| summed exactly in fp64 would need the budget itself)
    budget = oracle.spmm_csr(rowptr, colidx, np.abs(A0).astype(np.float64), np.abs(B0).astype(np.float64))
    assert longest * float(1 << bits_a) * float(1 << bits_b) <= 2.0 ** 53 and (budget < 2.0 ** 53).all(), "exact budget exceeded"
    val = np.ldexp(A0.astype(np.float64), (row_exp[rows] + col_exp[ci[:nnz]]).astype(np.int32))
    B = np.ldexp(B0.astype(np.float64), (-col_exp).astype(np.int32)[:, None])
    C0 = oracle.spmm_csr(rowptr, colidx, A0.astype(np.float64), B0.astype(np.float64))      # integers below 2^53: exact
    C_exact = np.ldexp(C0, row_exp.astype(np.int32)[:, None])
    return Exact(val, B, C_exact, A0, B0, row_exp, col_exp)


def exact_problem(rowptr, colidx, k, n, rng, wide):
    """(val, B, C_exact) for the pattern (rowptr, colidx) with k columns and an operand of n columns: see the module docstring."""
    return exact_parts(rowptr, colidx, k, n, rng, wide)[:3]


def rounded_problem(rowptr, colidx, k, n, rng):
    """(val, B) of ordinary rounded data on many scales: standard-normal values times 10^U(-12, 12) per row of A, standard-normal B times
    10^U(-6, 6) per row of B."""
    rp = np.asarray(rowptr, dtype=np.int64)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    val = rng.standard_normal(int(rp[-1])) * (10.0 ** rng.uniform(-12.0, 12.0, size=rp.size - 1))[rows]
    B = rng.standard_normal((k, n)) * (10.0 ** rng.uniform(-6.0, 6.0, size=k))[:, None]
    return val, B


def spmm_longdouble(rowptr, colidx, val, B):
    """A * B accumulated in np.longdouble, nonzeros in ascending order (one vectorised step per position in the row)."""
    rp = np.asarray(rowptr, dtype=np.int64)
    ci = np.asarray(colidx, dtype=np.int64)
    m = rp.size - 1
    v = np.asarray(val, dtype=np.longdouble)
    Bl = np.asarray(B, dtype=np.longdouble)
    lens = np.diff(rp)
    acc = np.zeros((m, Bl.shape[1]), dtype=np.longdouble)
    for t in range(int(lens.max()) if m else 0):
        rows = np.nonzero(lens > t)[0]
        p = rp[rows] + t
        acc[rows] += v[p][:, None] * Bl[ci[p]]
    return acc


def f64_bound(rowptr, colidx, val, B):
    """(ref, bound): ref = A * B in np.longdouble; bound(i, j) = 1.0001 (L_i + 1) 2^-53 (|A| |B|)(i, j) with L_i the row length.  Derived,
    not measured: gamma_L = L u / (1 - L u) covers any order (and any fusing) of an L-term dot product; the extra unit and the factor
    1.0001 cover the reference's own error (L 2^-64 (|A| |B|)), the rounding of |A| |B| itself and the 1 / (1 - L u)."""
    import oracle
    val = np.asarray(val, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    ref = spmm_longdouble(rowptr, colidx, val, B)
    absab = oracle.spmm_csr(rowptr, colidx, np.abs(val), np.abs(B))
    L = np.diff(np.asarray(rowptr, dtype=np.int64)).astype(np.float64)
    return ref, 1.0001 * (L[:, None] + 1.0) * U64 * absab


def check_f64_bound(rowptr, colidx, val, B, C, what="", ref_bound=None):
    """Assert that the fp64 product C (any summation order) of finite data meets |C - ref| <= 1.0001 (L_i + 1) 2^-53 (|A| |B|) entrywise
    against the np.longdouble reference, and that empty rows are exactly 0; no entry is left out.  On failure: the worst ratio and its
    (row, column).  ref_bound: f64_bound's result, when several products share it.  Returns the worst |C - ref| / bound."""
    ref, bound = f64_bound(rowptr, colidx, val, B) if ref_bound is None else ref_bound
    C = np.asarray(C)
    assert C.dtype == np.float64 and C.shape == ref.shape, (what, C.dtype, C.shape, ref.shape)
    assert np.isfinite(C).all(), (what, "C holds non-finite entries", np.argwhere(~np.isfinite(C))[:4].tolist())
    empty = np.diff(np.asarray(rowptr, dtype=np.int64)) == 0
    assert (C[empty] == 0).all(), (what, "an empty row is not exactly 0")
    err = np.abs(C.astype(np.longdouble) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)          # (bound 0 with an error: inf)
    worst = float(ratio.max()) if ratio.size else 0.0
    if (err > bound).any():
        i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s: fp64 error bound violated at %d entries; worst |C - ref| / bound = %.3g at (row %d, col %d): "
                             "C = %r, ref = %r, bound = %.3g" % (what, int((err > bound).sum()), ratio[i, j], i, j, C[i, j],
                                                                float(ref[i, j]), bound[i, j]))
    return worst
