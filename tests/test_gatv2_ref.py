"""CPU: the fixed order of the fused GATv2 attention (csrc/gatv2_kernels.hip), replayed in numpy (tests/gatv2_ref.replay), meets the
bound of DESIGN.md 5p on the inputs of tests/test_gpu_gatv2.py, forward and backward; the bound is tight enough to catch an entry
that is off by four bounds; the scores are rounded step by step; col_sum's order."""
import numpy as np
import pytest

import attention_ref as R
import gatv2_ref as G2
import softmax_ref as SR

DTYPES = ["float64", "float32"]
KEYS = G2.FWD_KEYS + G2.BWD_KEYS


def _got(out, keys):
    return {k: out[k] for k in keys}


def test_the_data_rule_holds_on_every_case():
    """5j's data rule, before anything else: T <= 60 in fp32, 600 in fp64, on the reference's own scores"""
    for dtype, H, dv, spread, short in G2.bound_cases():
        ref = G2.case(dtype, H, dv, spread, short)[-1]
        assert 0 < ref["T"] <= SR.T_MAX[np.dtype(dtype)], (dtype, H, dv, spread, ref["T"])
    for dtype in DTYPES:
        assert 40 < G2.steep_case(dtype)[-1]["T"] <= SR.T_MAX[np.dtype(dtype)]


def test_the_short_matrix_keeps_the_rows_the_wide_cases_rely_on():
    rp, ci, keep = G2.short_matrix()
    full_rp, full_ci = G2.matrix()
    lens = np.diff(rp)
    assert lens.max() == G2.SHORT and {0, 1, 7, 8, 9} <= set(lens.tolist())
    for k, r in enumerate(keep[:12]):
        assert np.array_equal(ci[rp[k]:rp[k + 1]], full_ci[full_rp[r]:full_rp[r + 1]])


@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_are_rounded_step_by_step(dtype):
    """the dtype scores differ from scores whose slope * z is not rounded before it meets a (a contracted product), and from the
    exact ones by less than the score error D"""
    dt = np.dtype(dtype)
    rp, ci = G2.matrix()
    XT, XS, a, _ = G2.operands(dtype, 1, 5, 3.0, 5)
    s, z, r = G2.scores_dtype(rp, ci, XT, XS, a, 0.2, 0)
    assert s.dtype == dt and z.dtype == dt and r.dtype == dt
    ld = np.longdouble
    sl = ld(dt.type(0.2))
    fused_r = np.where(z > 0, z.astype(ld), sl * z.astype(ld))          # z rounded, slope * z not
    lanes = R.group_of(5, dt)
    w = G2.W[dtype]
    acc = np.zeros((ci.size, lanes), ld)
    for j in range(5):
        lane = (j // w) % lanes
        acc[:, lane] = (ld(a[0, j]) * fused_r[:, j] + acc[:, lane]).astype(dt).astype(ld)     # one rounding per step
    k = 1
    while k < lanes:
        acc = (acc + acc[:, np.arange(lanes) ^ k]).astype(dt).astype(ld)
        k *= 2
    fused = acc[:, 0].astype(dt)
    assert ((s != fused) & (z < 0).any(axis=1)).any(), "the data can tell a contracted slope * z from a rounded one"
    assert not (s != fused)[(z > 0).all(axis=1)].any(), "where no slope is applied the two orders are one"
    exact, mag, _, _ = G2.scores_exact(rp, ci, XT, XS, a, 0.2, 0)
    assert (np.abs(s.astype(ld) - exact) <= 1.01 * (5 + 2) * SR.U[dt] * mag).all()


def test_slope_one_is_the_plain_dot_and_the_branch_is_exact():
    rp, ci = G2.matrix()
    XT, XS, a, _ = G2.operands("float64", 2, 8, 2.0, 9)
    rows = R.rows_of(rp)
    s1, z, r = G2.scores_dtype(rp, ci, XT, XS, a, 1.0, 1)
    assert np.array_equal(r, z) and np.array_equal(z, XT[rows, 8:] + XS[ci, 8:])
    want = R.dots_replay(np.broadcast_to(a[1][None, :], z.shape).copy(), z, 8)
    assert np.array_equal(s1, want)
    exact_z = XT[rows, 8:].astype(np.longdouble) + XS[ci, 8:].astype(np.longdouble)
    assert np.array_equal(z > 0, exact_z > 0), "the sign of fl(xt + xs) is the sign of the exact sum"


@pytest.mark.parametrize("dtype,H,dv,spread,short", list(G2.bound_cases()))
def test_replay_is_inside_the_bound(dtype, H, dv, spread, short):
    rp, ci, XT, XS, a, dO, ref = G2.case(dtype, H, dv, spread, short)
    out = G2.replay(rp, ci, XT, XS, a, G2.SLOPE, None, dO)
    r = G2.ratios(_got(out, KEYS), ref)
    print("replay, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s" % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype,H,dv,spread", list(G2.chunk_bound_cases()))
def test_replay_is_inside_the_bound_on_the_chunk_pattern(dtype, H, dv, spread):
    """rows of up to 200 entries and a hub column of 277: 5j's data rule on the reference alone, then the replay against the bound"""
    rp, ci, XT, XS, a, dO, ref = G2.chunk_case(dtype, H, dv, spread)
    assert 0 < ref["T"] <= SR.T_MAX[np.dtype(dtype)], (dtype, H, dv, spread, ref["T"])
    out = G2.replay(rp, ci, XT, XS, a, G2.SLOPE, None, dO)
    r = G2.ratios(_got(out, KEYS), ref)
    print("replay on the chunk pattern, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s"
          % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_of_the_steep_rows_with_bias(dtype):
    rp, ci, val, XT, XS, a, dO, ref = G2.steep_case(dtype)
    r = G2.ratios(_got(G2.replay(rp, ci, XT, XS, a, G2.SLOPE, val, dO), KEYS), ref)
    print("replay, steep rows with bias (%s): %s" % (dtype, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_entry_off_by_four_bounds_is_caught(dtype):
    """every output, one entry with a nonzero bound moved by four bounds: the ratio passes 1"""
    H, dv = 3, G2.widths(dtype)[3]
    rp, ci, XT, XS, a, dO, ref = G2.case(dtype, H, dv, G2.SPREADS[(3 + H) % 2])
    out = G2.replay(rp, ci, XT, XS, a, G2.SLOPE, None, dO)
    base = G2.ratios(_got(out, KEYS), ref)
    assert max(base.values()) <= 1
    for k in KEYS:
        want, bnd = ref[k]
        live = np.flatnonzero((bnd.ravel() > 0) & np.isfinite(want.ravel().astype(np.float64)))
        at = live[live.size // 2]
        bad = out[k].copy()
        step = 4 * float(bnd.ravel()[at])
        moved = bad.ravel()[at] + bad.dtype.type(step)
        assert abs(float(moved) - float(bad.ravel()[at])) >= 3 * float(bnd.ravel()[at]), (k, "the bound is below the dtype's spacing")
        bad.reshape(-1)[at] = moved
        assert G2.ratios({k: bad}, ref)[k] > 1, (dtype, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_col_sum_order(dtype):
    """blocks of 256 rows from +0 in ascending row, then the blocks left to right: exact data gives the exact sums, inexact data the
    bits of that order and of no other grouping; -0 columns come out as +0 (a block starts from +0)"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(3)
    for nrow in (0, 1, 255, 256, 257, 600):
        x = rng.integers(-50, 51, (nrow, 7)).astype(dt)
        assert np.array_equal(G2.col_sum_replay(x), x.sum(axis=0, dtype=np.float64).astype(dt))
    x = rng.standard_normal((600, 33)).astype(dt)
    got = G2.col_sum_replay(x)
    blocks = []
    for b in (slice(0, 256), slice(256, 512), slice(512, 600)):
        acc = np.zeros(33, dt)
        for row in x[b]:
            acc = acc + row
        blocks.append(acc)
    assert got.dtype == dt and np.array_equal(got, (blocks[0] + blocks[1]) + blocks[2])
    serial = np.zeros(33, dt)
    for row in x:
        serial = serial + row
    assert (got != serial).any(), "the data can tell the blocked order from one serial chain"
    bound = (255 + 3) * SR.U[dt] * np.abs(x).sum(axis=0)
    assert (np.abs(got.astype(np.longdouble) - x.astype(np.longdouble).sum(axis=0)) <= bound).all()
    z = G2.col_sum_replay(np.full((3, 2), -0.0, dt))
    assert (z == 0).all() and not np.signbit(z).any()
