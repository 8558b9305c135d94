"""CPU: the numpy replay of the fused attention kernel's fixed order (tests/attention_ref.py) stays inside the derived bound on
the very inputs of the GPU tests, and the bound is no wider than it says: an entry moved by 4 bounds is caught."""
import numpy as np
import pytest

import attention_ref as R


def _ratios(got, ref, dt):
    O, lse, p = got
    wo, _ = R.worst(O.ravel(), ref["O"].ravel(), R.bound_O(ref, dt).ravel())
    wp, _ = R.worst(p, ref["p"], R.bound_p(ref, dt))
    live = np.isfinite(ref["lse"].astype(np.float64))
    assert np.array_equal(np.isfinite(lse), live)
    wl, _ = R.worst(lse[live], ref["lse"][live], R.bound_lse(ref, dt)[live])
    return wo, wp, wl


@pytest.mark.parametrize("nk,nv,dtype", list(R.parity_cases()))
def test_replay_is_inside_the_bound(nk, nv, dtype):
    rp, ci, Q, K, V, scale, ref = R.case(nk, nv, dtype)
    wo, wp, wl = _ratios(R.replay(rp, ci, Q, K, V, scale), ref, dtype)
    print("replay %s nk=%d nv=%d: worst |err| / bound  O %.3g  p %.3g  lse %.3g" % (dtype, nk, nv, wo, wp, wl))
    assert wo <= 1 and wp <= 1 and wl <= 1, (wo, wp, wl)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_replay_on_the_rescale_rows(dtype):
    rp, ci, bias, Q, K, V, scale, ref = R.steep_case(dtype)
    O, lse, p = R.replay(rp, ci, Q, K, V, scale, bias.astype(dtype))
    wo, wp, wl = _ratios((O, lse, p), ref, dtype)
    print("replay %s steep rows: worst |err| / bound  O %.3g  p %.3g  lse %.3g" % (dtype, wo, wp, wl))
    assert wo <= 1 and wp <= 1 and wl <= 1, (wo, wp, wl)
    assert (p[~np.isfinite(bias)] == 0).all()


def test_scores_are_the_sddmm_group_bits_on_the_larger_group():
    """the dot of a narrow Q / K on the group a wide V asks for equals the dot on the SDDMM's own group, bit for bit"""
    rp, ci, Q, K, V, scale, ref = R.case(8, 40, "float64")
    assert R.group_of(8, Q.dtype) == 8 and R.lpr_of(8, 40, Q.dtype) == 32
    _, own = R.scores_replay(rp, ci, Q, K, 1.0)
    _, wide = R.scores_replay(rp, ci, Q, K, 1.0, lpr=32)
    assert np.array_equal(own, wide)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_an_entry_moved_by_four_bounds_is_caught(dtype):
    rp, ci, Q, K, V, scale, ref = R.case(33, 33, dtype)
    O, lse, p = R.replay(rp, ci, Q, K, V, scale)
    b = R.bound_O(ref, dtype)
    i, j = 8, 5                                             # the row of 200 entries
    assert b[i, j] > 0
    bad = O.copy()
    bad[i, j] = (bad[i, j].astype(np.longdouble) + 4 * b[i, j]).astype(O.dtype)
    w, at = R.worst(bad.ravel(), ref["O"].ravel(), b.ravel())
    assert w > 1 and at == i * O.shape[1] + j
