"""CPU checks of the fp32 references (tests/fp32_ref.py) the GPU fp32 kernel tests rely on: fma32 against exact rational
rounding, check_f32_bound accepting every summation order while rejecting each kind of subtle kernel bug, and
exact_problem32 giving one result in every order while a dropped nonzero or a misplaced B row shows."""
from fractions import Fraction

import numpy as np
import pytest

import fp32_ref as F


def _round_f32(x):
    """fp32 nearest (ties to even) of the rational x, by comparing the neighbours of a nearby fp32 exactly."""
    r = np.float32(float(x))
    cands = [np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))]
    best = None
    for c in cands:
        d = abs(Fraction(float(c)) - x)
        even = (int(np.array(c, dtype=np.float32).view(np.uint32)) & 1) == 0
        key = (d, not even)
        if best is None or key < best[0]:
            best = (key, c)
    return np.float32(best[1])


def _exact(a, b, c):
    return [_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)]


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_fma32_random_triples():
    rng = np.random.default_rng(1)
    N = 20000
    a = F.data_B(rng, N)
    b = F.data_B(rng, N)
    c = F.data_B(rng, N)
    # a quarter: c cancels most of a * b (results far below the inputs), a quarter of wide exponent range
    q = N // 4
    c[:q] = (-(a[:q].astype(np.float64) * b[:q]) * (1 + rng.uniform(-1e-6, 1e-6, q))).astype(np.float32)
    a[q:2 * q] = (rng.standard_normal(q) * np.exp2(rng.integers(-40, 40, q))).astype(np.float32)
    c[q:2 * q] = (rng.standard_normal(q) * np.exp2(rng.integers(-40, 40, q))).astype(np.float32)
    got = F.fma32(a, b, c)
    want = np.array(_exact(a, b, c), dtype=np.float32)
    assert np.array_equal(_bits(got), _bits(want))


def _midpoint_cases(rng, count):
    """Triples whose fp64 sum lands exactly on an fp32 midpoint while the exact sum lies off it (|tail| = j^2 2^-70 x scale): a = 1 + j 2^-23,
    b = +-2^-24 (1 - j 2^-23), so a * b = +-(2^-24 - j^2 2^-70).  c = r (odd significand, sum just below r's upper midpoint: exact result r)
    or c = r + ulp with r even (sum just above r's upper midpoint, negative product: exact result c).  Tie-to-even of the midpoint picks the
    wrong neighbour in both.  Scaled by powers of two and negated at random."""
    A, B, Cc, want = [], [], [], []
    for i in range(count):
        j = int(rng.integers(1, 180))
        sig = int(rng.integers(0, 1 << 22)) * 2            # even significand bits of r in [1, 2)
        below = i % 2 == 0
        if below:
            sig += 1                                       # r odd
        r = np.float32(1.0 + sig * 2.0 ** -23)
        a = np.float32(1.0 + j * 2.0 ** -23)
        b = np.float32(2.0 ** -24 * (1.0 - j * 2.0 ** -23))
        if below:
            c, res = r, r
        else:
            c, res, b = np.float32(r + np.float32(2.0 ** -23)), np.float32(r + np.float32(2.0 ** -23)), -b
        sc = 2.0 ** int(rng.integers(-20, 20))
        sg = -1.0 if rng.random() < 0.5 else 1.0
        A.append(np.float32(sg * sc * a)); B.append(b); Cc.append(np.float32(sg * sc * c)); want.append(np.float32(sg * sc * res))
    return (np.array(A, np.float32), np.array(B, np.float32), np.array(Cc, np.float32), np.array(want, np.float32))


def test_fma32_midpoints():
    rng = np.random.default_rng(2)
    a, b, c, want = _midpoint_cases(rng, 400)
    exact = np.array(_exact(a, b, c), dtype=np.float32)
    assert np.array_equal(_bits(exact), _bits(want))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert not (naive == want).any()                      # every case double-rounds wrongly: the midpoint path is exercised
    assert np.array_equal(_bits(F.fma32(a, b, c)), _bits(want))


def _rows(rng, m, k, maxlen):
    lens = rng.integers(0, maxlen + 1, size=m)
    lens[::7] = 0
    lens[1] = maxlen
    rp = np.zeros(m + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rng.choice(k, size=L, replace=False)) for L in lens]).astype(np.int32)
    return rp, ci, F.data_values(rng, ci.size)


def _f32_products(rp, ci, va, B, order):
    """fp32 numpy accumulation in a given order: 'asc', 'desc' (FMA chains) or 'pairwise' (products rounded, pairwise fp32 sums)."""
    v32 = va.astype(np.float32)
    m, n = rp.size - 1, B.shape[1]
    C = np.zeros((m, n), dtype=np.float32)
    for i in range(m):
        ps = list(range(rp[i], rp[i + 1]))
        if order == "desc":
            ps = ps[::-1]
        if order == "pairwise":
            terms = [(v32[p] * B[ci[p]]).astype(np.float32) for p in ps]
            while len(terms) > 1:
                terms = [(terms[t] + terms[t + 1]).astype(np.float32) if t + 1 < len(terms) else terms[t] for t in range(0, len(terms), 2)]
            C[i] = terms[0] if terms else 0.0
        else:
            acc = np.zeros(n, np.float32)
            for p in ps:
                acc = F.fma32(v32[p], B[ci[p]], acc)
            C[i] = acc
    return C


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(3)
    m, k, n = 60, 400, 16
    rp, ci, va = _rows(rng, m, k, 200)
    B = F.data_B(rng, (k, n))
    return rp, ci, va, B


def test_sequential_matches_fma_chain(case, orc):
    rp, ci, va, B = case
    C = F.csr_f32_sequential(rp, ci, va, B)
    assert np.array_equal(_bits(C), _bits(_f32_products(rp, ci, va, B, "asc")))
    # two sources: the same columns split into B0 / B1 give the same bits
    lo = 150
    B0, B1 = B[:lo], B[lo:]
    codes = np.where(ci < lo, ci, ~(ci - lo)).astype(np.int32)
    assert np.array_equal(_bits(F.csr_f32_sequential(rp, codes, va, B0, B1)), _bits(C))
    allneg = (~ci).astype(np.int32)
    assert np.array_equal(_bits(F.csr_f32_sequential(rp, allneg, va, None, B)), _bits(C))
    rowmap = np.arange(rp.size - 1) * 2 + 1
    R = F.csr_f32_sequential(rp, ci, va, B, rowmap=rowmap, nrow_c=2 * (rp.size - 1) + 1)
    assert np.array_equal(_bits(R[1::2]), _bits(C)) and np.isnan(R[0::2]).all()


@pytest.mark.parametrize("order", ["asc", "desc", "pairwise"])
def test_bound_accepts_every_order(case, orc, order):
    rp, ci, va, B = case
    F.check_f32_bound(rp, ci, va, B, _f32_products(rp, ci, va, B, order), order)


def _mutants(rp, ci, va, B, C):
    """(name, C') for each kind of subtle kernel bug the fp32 checks must catch."""
    lens = np.diff(rp)
    long_rows = np.nonzero((lens >= 3) & (lens <= 60))[0]
    i = int(long_rows[len(long_rows) // 2])
    # the mutated term: the row's largest value with a right neighbour of another magnitude in the same row
    cand = [q for q in range(int(rp[i]), int(rp[i + 1]) - 1) if abs(abs(va[q]) - abs(va[q + 1])) > 0.25 * abs(va[q])]
    p = max(cand, key=lambda q: abs(va[q]))
    v32 = va.astype(np.float32)
    out = []
    M = C.copy(); M[i] = (M[i].astype(np.float64) - v32[p].astype(np.float64) * B[ci[p]]).astype(np.float32)
    out.append(("one term dropped", M))
    M = C.copy(); M[i] = (M[i].astype(np.float64) + v32[p].astype(np.float64) * B[ci[p]]).astype(np.float32)
    out.append(("one term doubled", M))
    vn = va.copy(); vn[p] = va[p + 1]                       # a lane reading the neighbouring value slot
    out.append(("value from the neighbouring slot", F.csr_f32_sequential(rp, ci, vn, B)))
    j = int(long_rows[len(long_rows) // 2 + 1])
    M = C.copy(); M[[i, j]] = M[[j, i]]
    out.append(("two rows swapped", M))
    M = C.copy(); M[:, 4:8] = C[:, 5:9]                      # a 4-column piece read one column off
    out.append(("4-column piece shifted by one column", M))
    return out


def test_bound_rejects_mutants(case, orc):
    rp, ci, va, B = case
    C = F.csr_f32_sequential(rp, ci, va, B)
    F.check_f32_bound(rp, ci, va, B, C, "unmutated")
    names = []
    for name, M in _mutants(rp, ci, va, B, C):
        with pytest.raises(AssertionError, match="bound violated"):
            F.check_f32_bound(rp, ci, va, B, M, name)
        names.append(name)
    assert len(names) == 5


def test_bound_nonfinite_masks(orc):
    """Inf / NaN rows of B next to absent pairs: the masks must match the oracle's, finite entries stay bounded; a NaN leaking into a row
    that does not reference the bad B row is rejected."""
    rng = np.random.default_rng(5)
    rp, ci, va = _rows(rng, 40, 100, 30)
    B = F.data_B(rng, (100, 8))
    used = np.unique(ci)
    B[used[::9]] = np.inf
    B[used[4::13]] = np.nan
    C = F.csr_f32_sequential(rp, ci, va, B)
    F.check_f32_bound(rp, ci, va, B, C, "nonfinite")
    fin_rows = np.nonzero(np.isfinite(C).all(axis=1) & (np.diff(rp) > 0))[0]
    M = C.copy(); M[fin_rows[0], 3] = np.nan
    with pytest.raises(AssertionError, match="NaN positions"):
        F.check_f32_bound(rp, ci, va, B, M, "leaked NaN")


# ---- exact_problem32: data on which every fp32 summation order gives the same bits

@pytest.fixture(scope="module")
def exact32(orc):
    from crp_spmm_amd import gen
    rp, ci, _va = gen.random_csr(300, 260, 12, seed=4, empty_every=7)
    rng = np.random.default_rng(6)
    return (rp, ci) + F.exact_problem32(rp, ci, 260, 9, rng)


def test_exact32_is_normal_fp32_and_hits_both_scales(exact32):
    rp, ci, val, B, C = exact32
    assert val.dtype == np.float64 and B.dtype == np.float32 and C.dtype == np.float32
    assert np.array_equal(val.astype(np.float32).astype(np.float64), val)
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(val) >= tiny).all() and (np.abs(B) >= tiny).all() and (np.abs(C[C != 0]) >= tiny).all()
    assert (C[np.diff(rp) == 0] == 0).all() and (np.diff(rp) == 0).any()
    mag = np.abs(C[C != 0]).astype(np.float64)
    assert mag.max() / mag.min() > 2.0 ** 30             # rows of very different scales: what one norm cannot see


def test_exact32_every_order_gives_the_same_bits(exact32, orc):
    """(i) the kernel's ascending FMA chain, the same sum in reversed order and the fp64 oracle rounded to fp32."""
    rp, ci, val, B, C = exact32
    assert np.array_equal(_bits(F.csr_f32_sequential(rp, ci, val, B)), _bits(C))
    assert np.array_equal(_bits(_f32_products(rp, ci, val, B, "desc")), _bits(C))
    assert np.array_equal(_bits(_f32_products(rp, ci, val, B, "pairwise")), _bits(C))
    assert np.array_equal(_bits(orc.spmm_csr(rp, ci, val, B.astype(np.float64)).astype(np.float32)), _bits(C))


def test_exact32_shows_each_fault(exact32):
    """(ii) a dropped nonzero, two B rows swapped and a B row taken from the wrong source each change at least one entry."""
    rp, ci, val, B, C = exact32
    lens = np.diff(rp)
    i = int(np.nonzero(lens >= 3)[0][5])
    p = int(rp[i]) + 1
    dropped = val.copy(); dropped[p] = 0.0
    M = F.csr_f32_sequential(rp, ci, dropped, B)
    assert not np.array_equal(_bits(M), _bits(C)) and np.array_equal(_bits(np.delete(M, i, 0)), _bits(np.delete(C, i, 0)))
    c0, c1 = int(ci[p]), int(ci[p + 1])
    Bs = B.copy(); Bs[[c0, c1]] = Bs[[c1, c0]]                          # two received rows in each other's place
    assert not np.array_equal(_bits(F.csr_f32_sequential(rp, ci, val, Bs)), _bits(C))
    # two sources: columns [100, 200) local, the rest remote; the unmutated split gives C, remote position 0 read from B0 does not
    codes, remote = F.split_two_source(ci, 260, 100, 200)
    B0, B1 = B[100:200], B[remote]
    assert np.array_equal(_bits(F.csr_f32_sequential(rp, codes, val, B0, B1)), _bits(C))
    wrong = codes.copy()
    q = int(np.nonzero(codes < 0)[0][0])
    wrong[q] = ~codes[q]                                                # the same row number, taken from B0 instead of B1
    assert not np.array_equal(_bits(F.csr_f32_sequential(rp, wrong, val, B0, B1)), _bits(C))
    shifted = np.where(codes < 0, ~((~codes + 1) % remote.size), codes).astype(np.int32)   # every received row one row off
    assert not np.array_equal(_bits(F.csr_f32_sequential(rp, shifted, val, B0, B1)), _bits(C))
