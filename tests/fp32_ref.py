"""fp32 references for the fp32 SpMM kernels (helper module of the tests; not a conftest).

fma32              an exact, vectorised emulation of one single-rounded fp32 FMA (round to nearest even)
csr_f32_sequential the CSR row-group kernel's arithmetic (csrc/spmm_f32.hip) bit for bit
check_f32_bound    the error bound every summation order of the fp32 path meets, against the fp64 oracle
exact_problem32    data on which EVERY summation order, with or without FMA, gives the same fp32 bits (the twin of fp64_ref.exact_parts)

Data rule of the tests that use them: values and B entries are +-2^U(-8, 1) (data_values / data_B).  Every fp32 input is then a
multiple of 2^-31, so every exact product and partial sum is a multiple of 2^-62: a nonzero result stays far above the fp32
subnormal range (below 2^-126), and no test depends on the device's fp32 denormal mode.
"""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32


def data_values(rng, size):
    """+-2^U(-8, 1) in fp64 (rounded to fp32 by the library's conversion)."""
    return rng.choice((-1.0, 1.0), size=size) * np.exp2(rng.uniform(-8.0, 1.0, size=size))


def data_B(rng, shape):
    """+-2^U(-8, 1) as fp32."""
    return data_values(rng, shape).astype(np.float32)


ROW_EXP32, COL_EXP32 = 20, 10


def exact_problem32(rowptr, colidx, k, n, rng):
    """(val64, B32, C_exact32) for the pattern (rowptr, colidx) with k columns and an operand of n columns, on which every fp32
    summation order, fused or not, gives C_exact32 bit for bit -- the fp32 twin of fp64_ref.exact_parts.

    A = D_r A0 D_c and B = D_c^-1 B0 with power-of-two diagonals (row exponents uniform in [-20, 20], column exponents in
    [-10, 10]); A0 and B0 hold odd integers below 2^bits_a and 2^bits_b, bits_a + bits_b + ceil(log2(longest row)) <= 24.  Then
    val[p] * B[c][j] = a0 b0 2^(row exponent) exactly and sum_p |a0 b0| < 2^24 in every entry (asserted): every partial sum of every
    subset of a row's products is an integer below 2^24 times 2^(row exponent) -- exact in fp32.  |val| lies in [2^-30, 2^42),
    |B| in [2^-10, 2^22) and a nonzero |C| in [2^-20, 2^44): all normal fp32 numbers, so no result depends on the device's
    denormal mode.  val64 holds fp32-representable numbers: the library's fp64 -> fp32 conversion of the values is exact."""
    import oracle
    rp = np.asarray(rowptr, dtype=np.int64)
    ci = np.asarray(colidx, dtype=np.int64)
    m, nnz = rp.size - 1, int(rp[-1])
    assert nnz == 0 or (ci[:nnz].min() >= 0 and ci[:nnz].max() < k), "plain column indices (split two sources afterwards)"
    lens = np.diff(rp)
    longest = max(int(lens.max()) if m else 1, 1)
    room = 24 - int(np.ceil(np.log2(longest)))
    bits_a, bits_b = room // 2, room - room // 2
    assert bits_a >= 2, ("rows too long for the exact fp32 budget", longest)

    def odd(bits, size):
        mag = 2 * rng.integers(0, 1 << (bits - 1), size=size, dtype=np.int64) + 1
        return np.where(rng.integers(0, 2, size=size) == 1, mag, -mag)

    A0, B0 = odd(bits_a, nnz), odd(bits_b, (k, n))
    row_exp = rng.integers(-ROW_EXP32, ROW_EXP32 + 1, size=m)
    col_exp = rng.integers(-COL_EXP32, COL_EXP32 + 1, size=k)
    rows = np.repeat(np.arange(m), lens)
    budget = oracle.spmm_csr(rowptr, colidx, np.abs(A0).astype(np.float64), np.abs(B0).astype(np.float64))
    assert longest * float(1 << bits_a) * float(1 << bits_b) <= 2.0 ** 24 and (budget < 2.0 ** 24).all(), "exact fp32 budget exceeded"
    val64 = np.ldexp(A0.astype(np.float64), (row_exp[rows] + col_exp[ci[:nnz]]).astype(np.int32))
    B64 = np.ldexp(B0.astype(np.float64), (-col_exp).astype(np.int32)[:, None])
    C0 = oracle.spmm_csr(rowptr, colidx, A0.astype(np.float64), B0.astype(np.float64))      # integers below 2^24: exact
    C64 = np.ldexp(C0, row_exp.astype(np.int32)[:, None])
    B32, C32 = B64.astype(np.float32), C64.astype(np.float32)
    tiny = float(np.finfo(np.float32).tiny)
    assert np.array_equal(val64.astype(np.float32).astype(np.float64), val64) and np.array_equal(B32.astype(np.float64), B64) \
        and np.array_equal(C32.astype(np.float64), C64), "not exactly representable in fp32"
    assert (np.abs(val64) >= tiny).all() and (np.abs(B64) >= tiny).all() and (np.abs(C64[C64 != 0]) >= tiny).all(), "a subnormal"
    return val64, B32, C32


def fma32(a, b, c):
    """round_fp32(a * b + c) with ONE rounding, for fp32 arrays a, b, c (broadcast), as a float32 array.

    p = a * b is exact in fp64 (24 + 24 bits fit in 53); TwoSum gives s + e = p + c exactly; r = fp32(s).  Rounding s alone is
    right unless s is exactly midway between two fp32 neighbours: a midpoint is fp64-representable, so s + e (|e| <= ulp64(s) / 2)
    cannot lie across one.  At a midpoint with e != 0 the exact sum lies on e's side of it: r steps to that neighbour.  (Plain
    fp64-then-fp32 rounds twice and gets exactly those cases wrong.)  Non-finite inputs follow fp32(s)."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        d = s - r64                                            # exact (Sterbenz): s and r are neighbours
        fix = np.isfinite(s) & (d != 0) & np.isfinite(e) & (e != 0)
        if not fix.any():
            return r
        toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        q = np.nextafter(r, toward)                             # the other neighbour of s
        mid = fix & (2.0 * d == q.astype(np.float64) - r64)
        # exact sum on q's side of the midpoint (e has d's sign): q; else r
        return np.where(mid & ((e > 0) == (d > 0)), q, r).astype(np.float32)


def decode_cols(colidx):
    """Two-source column codes -> (source index 0 / 1, row in that source)."""
    ci = np.asarray(colidx, dtype=np.int64)
    neg = ci < 0
    return neg, np.where(neg, ~ci, ci)


def split_two_source(ci, k, lo, hi):
    """Columns [lo, hi) -> B0 rows (code c - lo), the rest -> B1 rows in ascending order (code ~position).  -> (codes, the B1 rows)."""
    remote = np.concatenate([np.arange(0, lo), np.arange(hi, k)])
    pos = np.full(k, -1)
    pos[remote] = np.arange(remote.size)
    codes = np.where((ci >= lo) & (ci < hi), ci - lo, ~pos[ci]).astype(np.int32)
    return codes, remote


def csr_f32_sequential(rowptr, codes, val64, B0, B1=None, rowmap=None, nrow_c=None):
    """What the CSR row-group kernel computes, bit for bit: acc = 0.0f; acc = fmaf(fp32(val[p]), B[col(p)][j], acc) for p in
    ascending order; codes < 0 read B1[~code].  val64 is rounded to fp32 to nearest even, as convert_f64_f32_kernel's (float) cast.
    rowmap: row i lands in row rowmap[i] of a (nrow_c, n) result (other rows NaN).  Vectorised over rows: one step per position."""
    rp = np.asarray(rowptr, dtype=np.int64)
    m = rp.size - 1
    v32 = np.asarray(val64, dtype=np.float64).astype(np.float32)
    n = (B0 if B0 is not None else B1).shape[1]
    parts = [np.asarray(X, dtype=np.float32).reshape(-1, n) for X in (B0, B1) if X is not None]
    Bs = np.concatenate(parts) if len(parts) > 1 else parts[0]          # [B0; B1]
    cols = single_source(codes, 0 if B0 is None else B0.shape[0])
    lens = np.diff(rp)
    acc = np.zeros((m, n), dtype=np.float32)
    for t in range(int(lens.max()) if m else 0):
        rows = np.nonzero(lens > t)[0]
        p = rp[rows] + t
        acc[rows] = fma32(v32[p][:, None], Bs[cols[p]], acc[rows])
    if rowmap is None:
        return acc
    out = np.full((nrow_c, n), np.nan, dtype=np.float32)
    out[np.asarray(rowmap)] = acc
    return out


def single_source(colidx, ncol0):
    """Two-source codes -> columns of the stacked operand [B0; B1] (B0 has ncol0 rows)."""
    neg, src = decode_cols(colidx)
    return np.where(neg, ncol0 + src, src).astype(np.int32)


def f32_bound(rowptr, colidx, val64, B32):
    """(ref, bound): ref = A * B in fp64 (oracle) on the fp64 values and fp32 B; bound(i, j) = 1.0001 (L_i + 1) 2^-24 (|A| |B|)(i, j)
    -- gamma for L_i products and additions, plus one rounding for the value conversion."""
    import oracle
    Bf = np.asarray(B32, dtype=np.float32).astype(np.float64)
    val64 = np.asarray(val64, dtype=np.float64)
    ref = oracle.spmm_csr(rowptr, colidx, val64, Bf)
    with np.errstate(invalid="ignore"):
        absab = oracle.spmm_csr(rowptr, colidx, np.abs(val64), np.abs(Bf))
    L = np.diff(np.asarray(rowptr, dtype=np.int64)).astype(np.float64)
    return ref, 1.0001 * (L[:, None] + 1.0) * U32 * absab


def check_f32_bound(rowptr, colidx, val64, B32, C, what="", ref_bound=None):
    """Assert that the fp32 product C (any summation order) meets |C - ref| <= 1.0001 (L_i + 1) 2^-24 (|A| |B|) entrywise, that
    empty rows are exactly 0, and (non-finite B) that C has the oracle's NaN and Inf positions; the bound holds for the finite
    entries.  On failure: the worst ratio and its (row, column).  ref_bound: f32_bound's result, when several products share it."""
    ref, bound = f32_bound(rowptr, colidx, val64, B32) if ref_bound is None else ref_bound
    C = np.asarray(C).astype(np.float64)
    assert C.shape == ref.shape, (what, C.shape, ref.shape)
    nan_ref, inf_ref = np.isnan(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(C), nan_ref), (what, "NaN positions differ from the fp64 oracle's")
    assert np.array_equal(np.isinf(C), inf_ref) and np.array_equal(np.sign(C[inf_ref]), np.sign(ref[inf_ref])), \
        (what, "Inf positions differ from the fp64 oracle's")
    empty = np.diff(np.asarray(rowptr, dtype=np.int64)) == 0
    assert (C[empty] == 0).all(), (what, "an empty row is not exactly 0")
    fin = np.isfinite(ref)
    err = np.where(fin, np.abs(C - np.where(fin, ref, 0.0)), 0.0)
    bad = err > np.where(fin, bound, np.inf)
    if bad.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(fin, err / bound, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s: fp32 error bound violated at %d entries; worst |C - ref| / bound = %.3g at (row %d, col %d): "
                             "C = %r, ref = %r, bound = %.3g" % (what, int(bad.sum()), ratio[i, j], i, j, C[i, j], ref[i, j],
                                                                bound[i, j]))
