"""CPU checks of the fp64 references (tests/fp64_ref.py) the GPU fp64 kernel tests rely on: the exact data really is exact (three
independent accumulations give C_exact bit for bit), check_f64_bound accepts the fp64 oracle on rounded data, and both checks reject each
kind of subtle kernel bug -- the first of which the suite's older bar, a relative Frobenius error of 1e-12, lets through."""
import numpy as np
import pytest

import fp64_ref as F


def _matrices():
    from crp_spmm_amd import gen
    nx, ny, nz = 300, 6, 5
    return [("random70", gen.random_csr(777, 1234, 70, seed=11, empty_every=13), 1234),
            ("random150", gen.random_csr(777, 1234, 150, seed=12, empty_every=13), 1234),
            ("kkt3d", gen.kkt3d(10), None), ("fem3d", gen.fem3d(12), None),
            ("lattice", gen.banded_fem(nx * ny * nz, offsets=(1, 2, 3, 4, 5, nx, nx + 1, nx * ny, nx * ny + 1), seed=4), None)]


MATRICES = {name: (rp, ci, k or rp.size - 1) for name, (rp, ci, _), k in _matrices()}


@pytest.mark.parametrize("wide", ["A", "B"])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_exact_problem_is_exact(orc, name, wide):
    """C_exact equals (1) an int64 accumulation of A0 B0 scaled by the row exponents, (2) the fp64 oracle on the scaled data and (3) a
    numpy accumulation of the scaled data over a random permutation of the nonzeros -- np.array_equal each.  Prints the share of C that a
    whole-matrix norm cannot see."""
    rp, ci, k = MATRICES[name]
    n = 33
    rng = np.random.default_rng(len(name) + (wide == "B"))
    P = F.exact_parts(rp, ci, k, n, rng, wide)
    m = rp.size - 1
    rows = np.repeat(np.arange(m), np.diff(rp))
    bits = int(np.abs(P.A0).max()).bit_length(), int(np.abs(P.B0).max()).bit_length()
    assert max(bits) == F.WIDE_BITS and (bits[0] > bits[1]) == (wide == "A"), bits
    assert (P.A0 % 2 != 0).all() and (P.B0 % 2 != 0).all()
    acc = np.zeros((m, n), dtype=np.int64)
    np.add.at(acc, rows, P.A0[:, None] * P.B0[ci])
    assert np.abs(acc).max() < (1 << 53)
    assert np.array_equal(np.ldexp(acc.astype(np.float64), P.row_exp.astype(np.int32)[:, None]), P.C_exact), "int64 accumulation"
    assert np.array_equal(orc.spmm_csr(rp, ci, P.val, P.B), P.C_exact), "fp64 oracle on the scaled data"
    perm = rng.permutation(ci.size)
    shuffled = np.zeros((m, n))
    np.add.at(shuffled, rows[perm], P.val[perm][:, None] * P.B[ci[perm]])
    assert np.array_equal(shuffled, P.C_exact), "permuted accumulation"
    assert not P.C_exact[np.diff(rp) == 0].any()
    # neither operand of the wide side survives fp32; every value of the narrow side does
    wide_arr, narrow_arr = (P.val, P.B) if wide == "A" else (P.B, P.val)
    assert (wide_arr.astype(np.float32).astype(np.float64) != wide_arr).mean() > 0.8
    assert np.array_equal(narrow_arr.astype(np.float32).astype(np.float64), narrow_arr)
    nz = np.abs(P.C_exact[P.C_exact != 0])
    rms = np.sqrt(np.mean(P.C_exact.astype(np.longdouble) ** 2))
    share = float((nz < 1e-12 * rms).mean())
    print("%s wide=%s: %.1f %% of the nonzero entries of C lie below 1e-12 x RMS" % (name, wide, 100 * share))
    assert share > 0.25            # the row exponents span 2^+-40: a good part of C is invisible to a whole-matrix norm


def test_second_value_set_keeps_exponents_and_B():
    rp, ci, k = MATRICES["kkt3d"]
    P = F.exact_parts(rp, ci, k, 8, np.random.default_rng(1), "A")
    Q = F.exact_parts(rp, ci, k, 8, np.random.default_rng(2), "A", like=P)
    assert Q.B is not P.B and np.array_equal(Q.B, P.B) and np.array_equal(Q.row_exp, P.row_exp) and np.array_equal(Q.col_exp, P.col_exp)
    assert not np.array_equal(Q.A0, P.A0) and not np.array_equal(Q.C_exact, P.C_exact)


def _faults(rp, ci, val, B, scale_rows, scale_brows, rng):
    """The injected kernel bugs, as (name, val', B', edit of C): each changes the inputs the oracle multiplies, or the product itself.
    scale_rows / scale_brows: the scale of every row of A / of B (the faults go where the data is small)."""
    lens = np.diff(rp)
    small_row = min((r for r in range(lens.size) if lens[r] >= 2), key=lambda r: scale_rows[r])
    p0, p1 = int(rp[small_row]), int(rp[small_row + 1])
    out = []
    v = val.copy()
    v[p0 + (p1 - p0) // 2] = 0.0
    out.append(("a nonzero of the smallest-scaled row dropped", v, B, None))
    used = np.unique(ci)
    c1, c2 = used[np.argsort(scale_brows[used])[:2]]
    Bs = B.copy()
    Bs[[c1, c2]] = Bs[[c2, c1]]
    out.append(("two B rows of small scale swapped", val, Bs, None))
    v = val.copy()
    changes = np.nonzero(v[p0:p1].astype(np.float32).astype(np.float64) != v[p0:p1])[0]
    q = p0 + int(changes[np.argmax(np.abs(v[p0:p1][changes]))])
    v[q] = np.float64(np.float32(v[q]))
    out.append(("one value rounded to fp32", v, B, None))

    def edge(C):
        C = C.copy()
        C[:, 128] = C[:, 127]
        return C
    out.append(("column 127 of C copied into column 128", val, B, edge))
    v = val.copy()
    v[[p0, p0 + 1]] = v[[p0 + 1, p0]]
    out.append(("one value moved to the neighbouring slot", v, B, None))
    return out


@pytest.mark.parametrize("name", ["random150", "kkt3d"])
def test_checks_bite(orc, name):
    """Each injected fault fails np.array_equal against C_exact on the exact data AND check_f64_bound on the rounded data, while the
    unharmed oracle passes both; the first fault stays within rel_fro_err <= 1e-12 on both data sets -- the gap these checks close."""
    rp, ci, k = MATRICES[name]
    n = 130
    rng = np.random.default_rng(5)
    P = F.exact_parts(rp, ci, k, n, rng, "A")
    val, B = F.rounded_problem(rp, ci, k, n, rng)
    rb = F.f64_bound(rp, ci, val, B)
    worst = F.check_f64_bound(rp, ci, val, B, orc.spmm_csr(rp, ci, val, B), "the fp64 oracle", ref_bound=rb)
    print("%s: the fp64 oracle's worst |C - ref| / bound = %.3g" % (name, worst))
    assert worst <= 1.0
    lens = np.diff(rp)
    rows = np.repeat(np.arange(lens.size), lens)
    row_scale = np.zeros(lens.size)
    np.maximum.at(row_scale, rows, np.abs(val))
    exact_faults = _faults(rp, ci, P.val, P.B, P.row_exp.astype(np.float64), -P.col_exp.astype(np.float64), rng)
    rounded_faults = _faults(rp, ci, val, B, row_scale, np.abs(B).max(axis=1), rng)
    for i, ((what, ve, Be, edit_e), (_, vr, Br, edit_r)) in enumerate(zip(exact_faults, rounded_faults)):
        Ce = orc.spmm_csr(rp, ci, ve, Be)
        Ce = edit_e(Ce) if edit_e else Ce
        assert not np.array_equal(Ce, P.C_exact), (what, "passes the exact comparison")
        Cr = orc.spmm_csr(rp, ci, vr, Br)
        Cr = edit_r(Cr) if edit_r else Cr
        with pytest.raises(AssertionError, match="fp64 error bound violated"):
            F.check_f64_bound(rp, ci, val, B, Cr, what, ref_bound=rb)
        if i == 0:
            fro_e = orc.rel_fro_err(P.C_exact, Ce)
            fro_r = orc.rel_fro_err(np.asarray(rb[0], dtype=np.float64), Cr)
            print("%s: %s: rel_fro_err %.3g (exact data), %.3g (rounded data)" % (name, what, fro_e, fro_r))
            assert fro_e <= 1e-12 and fro_r <= 1e-12, (what, "the whole-matrix norm sees it after all", fro_e, fro_r)


def test_check_f64_bound_reports_location_and_empty_rows(orc):
    rp, ci, k = MATRICES["random70"]
    rng = np.random.default_rng(9)
    val, B = F.rounded_problem(rp, ci, k, 5, rng)
    C = orc.spmm_csr(rp, ci, val, B)
    rb = F.f64_bound(rp, ci, val, B)
    assert F.check_f64_bound(rp, ci, val, B, C, ref_bound=rb) <= 1.0
    bad = C.copy()
    bad[17, 3] *= 1.0 + 2.0 ** -40
    with pytest.raises(AssertionError, match=r"\(row 17, col 3\)"):
        F.check_f64_bound(rp, ci, val, B, bad, "one entry off", ref_bound=rb)
    bad = C.copy()
    bad[13, 0] = 1e-300
    with pytest.raises(AssertionError, match="empty row"):
        F.check_f64_bound(rp, ci, val, B, bad, ref_bound=rb)
