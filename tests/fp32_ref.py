"""fp32 references for the fp32 SpMM kernels (helper module of the tests; not a conftest).

fma32              an exact, vectorised emulation of one single-rounded fp32 FMA (round to nearest even)
csr_f32_sequential the CSR row-group kernel's arithmetic (csrc/spmm_f32.hip) bit for bit
check_f32_bound    the error bound every summation order of the fp32 path meets, against the fp64 oracle

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
