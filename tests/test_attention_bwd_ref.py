"""CPU: the numpy replay of the fused attention backward's fixed order (tests/attention_bwd_ref.py) stays inside the derived
bounds on the very inputs of the GPU tests, the bounds are no wider than they say (a gradient entry moved by four bounds is
caught), and the reference is the gradient torch autograd forms on the dense masked attention."""
import numpy as np
import pytest

import attention_bwd_ref as B
import attention_ref as R

KEYS = ("dQ", "dK", "dV", "ds", "delta")


def test_the_pattern_has_what_the_tests_rely_on():
    B.check_matrix()


@pytest.mark.parametrize("nk,nv,dtype", list(B.parity_cases()))
def test_replay_is_inside_the_bounds(nk, nv, dtype):
    rp, ci, nrow, Q, K, V, dO, scale, ref = B.case(nk, nv, dtype)
    O, lse, _ = R.replay(rp, ci, Q, K, V, scale)                # the forward's outputs in the dtype: the backward's inputs
    got = B.replay(rp, ci, Q, K, V, O, lse, dO, scale)
    w = B.ratios({k: got[k] for k in KEYS}, ref, dtype)
    print("replay %s nk=%d nv=%d: worst |err| / bound  %s" % (dtype, nk, nv, "  ".join("%s %.3g" % (k, w[k]) for k in KEYS)))
    assert all(w[k] <= 1 for k in KEYS), w
    empty = np.diff(rp) == 0
    assert (got["dQ"][empty] == 0).all() and not np.signbit(got["dQ"][empty]).any()
    one = np.flatnonzero(np.diff(rp) == 1)
    assert (got["ds"][rp[one]] == 0).all(), "a one-entry row has p = 1 and dP = delta"


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_replay_on_the_rescale_rows(dtype):
    rp, ci, bias, Q, K, V, scale, _ = R.steep_case(dtype)
    dO = np.random.default_rng(9).standard_normal((Q.shape[0], V.shape[1])).astype(dtype)
    ref = B.reference(rp, ci, Q, K, V, dO, scale, bias.astype(dtype))
    O, lse, _ = R.replay(rp, ci, Q, K, V, scale, bias.astype(dtype))
    got = B.replay(rp, ci, Q, K, V, O, lse, dO, scale, bias.astype(dtype))
    w = B.ratios({k: got[k] for k in KEYS}, ref, dtype)
    print("replay %s steep rows: worst |err| / bound  %s" % (dtype, w))
    assert all(w[k] <= 1 for k in KEYS), w
    assert (got["ds"][~np.isfinite(bias)] == 0).all() and (got["p"][~np.isfinite(bias)] == 0).all()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("key", ["dQ", "dK", "dV", "ds"])
def test_a_gradient_entry_moved_by_four_bounds_is_caught(dtype, key):
    rp, ci, nrow, Q, K, V, dO, scale, ref = B.case(33, 32, dtype)
    O, lse, _ = R.replay(rp, ci, Q, K, V, scale)
    got = B.replay(rp, ci, Q, K, V, O, lse, dO, scale)
    bound = dict(dQ=B.bound_dQ, dK=B.bound_dK, dV=B.bound_dV, ds=B.bound_ds)[key](ref, dtype)
    at = {"dQ": (8, 5), "dK": (B.HUB, 5), "dV": (B.HUB, 5), "ds": (int(rp[8]) + 3,)}[key]      # the row of 200 entries, the hub column
    assert bound[at] > 0
    bad = got[key].copy()
    bad[at] = (bad[at].astype(np.longdouble) + 4 * bound[at]).astype(bad.dtype)
    w, where = B.worst(bad.ravel(), ref[key].ravel(), np.asarray(bound).ravel())
    assert w > 1 and where == np.ravel_multi_index(at, bad.shape)
    assert B.ratios({key: got[key]}, ref, dtype)[key] <= 1


def test_the_reference_is_torch_autograd_on_the_dense_masked_attention():
    rp, ci, Q, K, V, dO, scale = B.dense_case()
    ref = B.reference(rp, ci, Q, K, V, dO, scale)
    for key, want in zip(("dQ", "dK", "dV"), B.dense_autograd(rp, ci, Q, K, V, dO, scale)):
        # autograd rounds in fp64 (m = 64: sums of at most 64 terms of size O(1)); the reference is exact
        assert np.abs(ref[key].astype(np.float64) - want).max() <= 1e-13, key
