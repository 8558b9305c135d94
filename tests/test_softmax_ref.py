"""CPU: the numpy replay of the row softmax's fixed summation order (tests/softmax_ref.py) meets the derived error bounds on
the very inputs the GPU tests use (tests/test_gpu_row_softmax.py), so the reference order alone stays inside both bounds; the
special cases hold in the replay; and the test data keeps the data rule."""
import numpy as np
import pytest

import softmax_ref as R

DTYPES = (np.float64, np.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp64", "fp32"))
def test_replay_meets_both_bounds_on_the_gpu_tests_inputs(crp, dtype):
    top_f = top_b = 0.0
    for name, spread in R.parity_cases():
        rp, s, ref, bound, y, dy, ref_b, bound_b = R.case(name, spread, dtype)
        wf, at = R.worst(y, ref, bound)
        assert wf <= 1.0, (name, spread, "forward", wf, at)
        wb, at = R.worst(R.replay_bwd(rp, y, dy), ref_b, bound_b)
        assert wb <= 1.0, (name, spread, "backward", wb, at)
        top_f, top_b = max(top_f, wf), max(top_b, wb)
    print("%s: worst |err| / bound of the replay: forward %.3g, backward %.3g" % (np.dtype(dtype).name, top_f, top_b))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp64", "fp32"))
def test_data_rule_and_special_cases(crp, dtype):
    tiny = np.finfo(dtype).tiny
    for name, spread in R.parity_cases():
        rp, s, ref, bound, y, dy, ref_b, bound_b = R.case(name, spread, dtype)
        lens = np.diff(rp)
        masked = np.isneginf(s)
        assert masked.sum() == (lens >= 2).sum()
        assert (y[masked] == 0).all() and (ref[masked] == 0).all()
        assert (y[~masked] > 1e6 * tiny).all(), (name, spread)            # nothing near the subnormal range
        assert (y[rp[:-1][lens == 1]] == 1).all()
        assert np.isfinite(y).all()


def test_all_masked_row_and_single_entries():
    rp = R.rowptr_of([3, 0, 1, 1, 70])
    for dtype in DTYPES:
        s = np.concatenate([[-np.inf] * 3, [5.0], [-np.inf], np.linspace(-4, 4, 70)]).astype(dtype)
        y = R.replay_fwd(rp, s)
        ref, _L, _T = R.reference_fwd(rp, s)
        assert (y[:3] == 0).all() and y[3] == 1 and y[4] == 0 and np.isfinite(y).all()
        assert (ref[:3] == 0).all() and ref[3] == 1 and ref[4] == 0


def test_the_row_pointers_sit_either_side_of_every_lane_group_threshold():
    assert R.lpr_of(R.pattern("synthetic")) == 64
    for (k, over, lpr), name in zip(R.LPR_EDGES, R.EDGE_PATTERNS):
        rp = R.pattern(name)
        assert R.lpr_of(rp) == lpr, (name, R.lpr_of(rp))
        assert int(rp[-1]) == k * (rp.size - 1) + (1 if over else 0)
        assert tuple(np.diff(rp)[:len(R.SYNTH_LENGTHS)]) == R.SYNTH_LENGTHS


def test_a_row_subset_replays_to_the_same_bits():
    rp, s, *_ = R.case("synthetic", 8, np.float32)
    full = R.replay_fwd(rp, s)
    sub = rp[40:90]
    assert np.array_equal(R.replay_fwd(sub, s), full[sub[0]:sub[-1]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replays_fma_rounds_once(dtype):
    """softmax_ref.fma against exact rational arithmetic: random operands, cancelling ones, and sums that land exactly half way
    between two numbers of the dtype after the wider rounding (the cases a product-then-sum emulation gets wrong)."""
    from fractions import Fraction
    dt = np.dtype(dtype)
    bits = 53 if dt == np.float64 else 24
    rng = np.random.default_rng(9)
    n = 4000
    a = rng.standard_normal(n).astype(dt)
    b = rng.standard_normal(n).astype(dt)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 31, n))).astype(dt)
    c[:500] = -(a[:500] * b[:500])                                       # cancellation: the low half of the product survives
    # ties: c = 1 + one ulp (odd last bit), a * b = half an ulp less 2^-2j of it, too little for the wider format to keep: the
    # wider sum lands exactly half way and goes to the even neighbour above, the exact sum lies below the half
    j = rng.integers(15, 24, 500).astype(np.float64)
    a[500:1000] = (np.ldexp(1.0, -(bits // 2)) * (1 + np.exp2(-j))).astype(dt)
    b[500:1000] = (np.ldexp(1.0, -(bits - bits // 2)) * (1 - np.exp2(-j))).astype(dt)
    c[500:1000] = np.asarray(1 + np.ldexp(1.0, 1 - bits), dt)
    a[750:1000], c[750:1000] = -a[750:1000], -c[750:1000]
    got = R.fma(a, b, c)
    assert got.dtype == dt

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        if v == 0:
            return dt.type(0.0)
        if dt == np.float64:
            return np.float64(float(v))                                  # int / int division of a Fraction rounds correctly
        sign, v = (-1, -v) if v < 0 else (1, v)
        e = v.numerator.bit_length() - v.denominator.bit_length()
        e = e if v >= Fraction(2) ** e else e - 1
        q = v / Fraction(2) ** (e - bits + 1)                           # 2^(bits - 1) <= q < 2^bits
        fl = q.numerator // q.denominator
        rem = q - fl
        fl += 1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1) else 0
        return np.float32(sign * float(fl) * 2.0 ** (e - bits + 1))

    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], dt)
    assert np.array_equal(got, want), int((got != want).sum())
    naive = (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(dt) if dt == np.float64 else \
        (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(dt)
    assert (naive != want).any()                                         # the data holds cases that need the single rounding
