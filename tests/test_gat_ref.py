"""CPU: the fixed order of the fused GAT attention (csrc/gat_kernels.hip), replayed in numpy (tests/gat_ref.replay), meets the bound
of DESIGN.md 5o on the inputs of tests/test_gpu_gat.py, forward and backward, and the bound is tight enough to catch an entry that
is off by four bounds."""
import numpy as np
import pytest

import gat_ref as G

DTYPES = ["float64", "float32"]


def _got(out, keys):
    return {k: out[k] for k in keys}


def test_the_matrix_has_the_rows_the_tests_rely_on():
    rp, ci = G.matrix()
    lens = np.diff(rp)
    assert rp.size - 1 == G.NROW and set(G.SPECIAL_LENGTHS) <= set(lens.tolist()) and lens.max() == 70
    assert np.bincount(ci, minlength=G.NCOL)[G.EMPTY_COL] == 0
    codes = G.two_source_codes(ci)
    assert (codes < 0).any() and (codes >= 0).any() and (~codes[codes < 0]).max() < G.NCOL - G.K0


def test_scores_are_rounded_step_by_step():
    """the dtype scores differ from a contracted slope * z + val where that differs: the data of the bias pin can tell the two apart"""
    rp, ci = G.matrix()
    el, er, _, _ = G.operands("float32", 1, 1, 3.0, 5)
    val = np.random.default_rng(1).standard_normal(ci.size)
    s, g = G.scores_dtype(rp, ci, el, er, 0.2, 0, val)
    rows = np.repeat(np.arange(G.NROW), np.diff(rp))
    z = (el[rows, 0] + er[ci, 0]).astype(np.float32)
    fused = np.where(z > 0, z.astype(np.float64) + val.astype(np.float32), np.float64(np.float32(0.2)) * z + val.astype(np.float32)).astype(np.float32)
    assert s.dtype == np.float32 and (s != fused).any() and np.abs(s - fused).max() < 1e-5
    assert set(np.unique(g).tolist()) == {float(np.float32(0.2)), 1.0}


@pytest.mark.parametrize("dtype,H,dv,spread", list(G.bound_cases()))
def test_replay_is_inside_the_bound(dtype, H, dv, spread):
    rp, ci, el, er, V, dO, ref = G.case(dtype, H, dv, spread)
    out = G.replay(rp, ci, el, er, V, G.SLOPE, None, dO)
    r = G.ratios(_got(out, G.FWD_KEYS + G.BWD_KEYS), ref)
    print("replay, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s" % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_of_the_steep_rows_and_of_the_second_block(dtype):
    rp, ci, val, el, er, V, dO, ref = G.steep_case(dtype)
    r = G.ratios(_got(G.replay(rp, ci, el, er, V, G.SLOPE, val, dO), G.FWD_KEYS + G.BWD_KEYS), ref)
    print("replay, steep rows with bias (%s): %s" % (dtype, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r
    rp, ci, el, er, V, ref = G.second_block_case(dtype)
    r = G.ratios(_got(G.replay(rp, ci, el, er, V, G.SLOPE), G.FWD_KEYS), ref)
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_entry_off_by_four_bounds_is_caught(dtype):
    """every output, one entry with a nonzero bound moved by four bounds: the ratio passes 1"""
    H, dv = 3, G.widths(dtype)[3]
    rp, ci, el, er, V, dO, ref = G.case(dtype, H, dv, G.SPREADS[(3 + H) % 2])
    out = G.replay(rp, ci, el, er, V, G.SLOPE, None, dO)
    base = G.ratios(_got(out, G.FWD_KEYS + G.BWD_KEYS), ref)
    assert max(base.values()) <= 1
    for k in G.FWD_KEYS + G.BWD_KEYS:
        want, bnd = ref[k]
        live = np.flatnonzero((bnd.ravel() > 0) & np.isfinite(want.ravel().astype(np.float64)))
        at = live[live.size // 2]
        bad = out[k].copy()
        step = 4 * float(bnd.ravel()[at])
        moved = bad.ravel()[at] + bad.dtype.type(step)
        assert abs(float(moved) - float(bad.ravel()[at])) >= 3 * float(bnd.ravel()[at]), (k, "the bound is below the dtype's spacing")
        bad.reshape(-1)[at] = moved
        assert G.ratios({k: bad}, ref)[k] > 1, (dtype, k)


def test_slope_one_is_the_plain_additive_score_and_slope_zero_masks_nothing():
    rp, ci = G.matrix()
    el, er, _, _ = G.operands("float64", 2, 1, 2.0, 9)
    rows = np.repeat(np.arange(G.NROW), np.diff(rp))
    s1, g1 = G.scores_dtype(rp, ci, el, er, 1.0, 1)
    assert np.array_equal(s1, el[rows, 1] + er[ci, 1]) and (g1 == 1).all()
    s0, g0 = G.scores_dtype(rp, ci, el, er, 0.0, 0)
    assert (s0 >= 0).all() and np.isfinite(s0).all() and set(np.unique(g0).tolist()) == {0.0, 1.0}
