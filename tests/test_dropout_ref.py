"""CPU: the attention-dropout mask (csrc/dropout.h) against a numpy Philox4x32-10 and its known answers, the fixture the GPU tests
run under, and the fixed order of the dropped GAT / GATv2 attention replayed in numpy (tests/dropout_ref) against the bound of
DESIGN.md 5q, forward and backward; the bound is tight enough to catch an entry that is off by four bounds."""
import ctypes as C

import numpy as np
import pytest

import dropout_ref as D
import gat_ref as G
import gatv2_ref as G2
import softmax_ref as SR

DTYPES = ["float64", "float32"]
GAT_KEYS = G.FWD_KEYS + G.BWD_KEYS
GATV2_KEYS = G2.FWD_KEYS + G2.BWD_KEYS


def _got(out, keys):
    return {k: out[k] for k in keys}


def test_philox_known_answers():
    for ctr, key, want in D.KNOWN_ANSWERS:
        got = tuple(int(x) for x in D.philox4x32_10(*ctr, *key))
        assert got == want, ([hex(x) for x in got], [hex(x) for x in want])


def test_threshold_and_scale():
    assert D.threshold(0.0) == 0 and D.threshold(2.0 ** -33) == 0 and D.threshold(0.5) == 1 << 31
    assert D.threshold(1 - 2.0 ** -32) == (1 << 32) - 1 and D.threshold(1 - 2.0 ** -53) == (1 << 32) - 1
    assert D.rs_of(0.5, "float32") == 2 and D.rs_of(0.6, "float64") == 1.0 / (1.0 - 0.6)
    assert D.rs_of(0.6, "float32") == np.float32(1.0 / (1.0 - 0.6)) and D.rs_of(2.0 ** -33, "float64") > 1


def test_the_host_function_is_the_numpy_draw():
    """crp_dropout_keep_host over a grid of (seed, r, c, h, drop): column codes with the top bit set (a second-source code goes in
    as its bit pattern), both words of the seed, and the rates at which the threshold is 0, 2^31 and 2^32 - 1"""
    from crp_spmm_amd import _lib as L
    from crp_spmm_amd import hip
    fn = L.load().crp_dropout_keep_host
    seeds = (0, 1, 0xFFFFFFFF, 1 << 32, D.SEED, (1 << 64) - 1)
    rs_ = (0, 1, 39, 0x7FFFFFFF, 0xFFFFFFFF)
    cs = (0, 5, 79, 0x80000000, 0xFFFFFFFE, int(np.uint32(np.int32(~3))))
    drops = (0.0, 2.0 ** -33, 0.1, 0.5, 0.6, 1 - 2.0 ** -32)
    n = 0
    for seed in seeds:
        for drop in drops:
            want = D.keep(seed, np.array(rs_)[:, None, None], np.array(cs)[None, :, None], np.arange(4)[None, None, :], drop)
            for i, r in enumerate(rs_):
                for j, c in enumerate(cs):
                    for h in range(4):
                        got = fn(seed, r, c, h, drop)
                        assert got in (0, 1) and bool(got) == bool(want[i, j, h]), (seed, r, c, h, drop)
                        n += 1
            if drop <= 2.0 ** -33:
                assert want.all()                       # below 2^-32 every edge is kept
    assert n == len(seeds) * len(drops) * len(rs_) * len(cs) * 4
    # the wrapper takes a negative code as its bit pattern
    assert hip.dropout_keep(D.SEED, 3, -4, 1, 0.5) == bool(D.keep(D.SEED, 3, -4, 1, 0.5)) == bool(D.keep(D.SEED, 3, 0xFFFFFFFC, 1, 0.5))


@pytest.mark.parametrize("drop", [0.1, 0.5, 0.6])
def test_kept_share_over_2_20_keys(drop):
    """the kept share of 2^20 keys lies within 5 sigma of 1 - thr / 2^32 (the draws are deterministic: a fixed fact)"""
    n = 1 << 20
    i = np.arange(n)
    k = D.keep(D.SEED, i >> 10, i & 1023, i % 3, drop)
    q = 1.0 - D.threshold(drop) / 2.0 ** 32
    sigma = np.sqrt(q * (1 - q) / n)
    share = k.mean()
    print("drop %.1f: kept share %.6f, expected %.6f, %.2f sigma" % (drop, share, q, abs(share - q) / sigma))
    assert abs(share - q) <= 5 * sigma


def test_fixture():
    """under (DROP, SEED) every row of the test matrix with 8 or more entries has a kept and a dropped entry in every head, and a
    row of 2 or more entries is wholly dropped in some head -- on the reference alone"""
    mixed, wholly = D.fixture_facts()
    assert mixed and wholly, (mixed, wholly)
    assert (8, 1) in wholly                             # the row the GPU tests name
    rp, ci = G.matrix()
    assert rp[9] - rp[8] >= 2
    # heads differ, seeds differ, and the transposed pair sees the same bits
    k = D.mask_csr(rp, ci, D.HEADS, D.DROP, D.SEED)
    assert (k[:, 0] != k[:, 1]).any() and (k != D.mask_csr(rp, ci, D.HEADS, D.DROP, D.SEED + 1)).any()


@pytest.mark.parametrize("dtype,H,dv,spread", list(D.gat_bound_cases()))
def test_gat_replay_is_inside_the_bound(dtype, H, dv, spread):
    rp, ci, el, er, V, dO, ref = D.gat_case(dtype, H, dv, spread)
    out = D.gat_replay(rp, ci, el, er, V, G.SLOPE, D.DROP, D.SEED, None, dO)
    r = D.ratios(_got(out, GAT_KEYS), ref)
    print("GAT replay under dropout, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s"
          % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r
    # lse and p are the replay's without dropout, bit for bit
    plain = G.replay(rp, ci, el, er, V, G.SLOPE)
    assert np.array_equal(out["lse"], plain["lse"]) and np.array_equal(out["p"], plain["p"])


@pytest.mark.parametrize("dtype,H,dv,spread,short", list(D.gatv2_bound_cases()))
def test_gatv2_replay_is_inside_the_bound(dtype, H, dv, spread, short):
    rp, ci, XT, XS, a, dO, ref = D.gatv2_case(dtype, H, dv, spread, short)
    out = D.gatv2_replay(rp, ci, XT, XS, a, G2.SLOPE, D.DROP, D.SEED, None, dO)
    r = D.ratios(_got(out, GATV2_KEYS), ref)
    print("GATv2 replay under dropout, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s"
          % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r


def test_chunk_fixture():
    """under (DROP, SEED) on the chunk pattern every full chunk after the first of a row, and of the hub column, holds other keep bits
    than the first, at every chunk size: a kernel that takes them from the wrong chunk takes wrong ones"""
    ok, hub = D.chunk_fixture_facts()
    assert ok and hub > 4 * 64 + 8, (ok, hub)


@pytest.mark.parametrize("dtype,H,dv,spread,backward", list(G.chunk_bound_cases()))
def test_gat_replay_is_inside_the_bound_on_the_chunk_pattern(dtype, H, dv, spread, backward):
    rp, ci, el, er, V, dO, ref = D.gat_chunk_case(dtype, H, dv, spread, backward)
    assert 0 < ref["T"] <= SR.T_MAX[np.dtype(dtype)], (dtype, H, dv, spread, ref["T"])
    out = D.gat_replay(rp, ci, el, er, V, G.SLOPE, D.DROP, D.SEED, None, dO)
    r = D.ratios(_got(out, G.FWD_KEYS + (G.BWD_KEYS if backward else ())), ref)
    print("GAT replay under dropout on the chunk pattern, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s"
          % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype,H,dv,spread", list(G2.chunk_bound_cases()))
def test_gatv2_replay_is_inside_the_bound_on_the_chunk_pattern(dtype, H, dv, spread):
    rp, ci, XT, XS, a, dO, ref = D.gatv2_chunk_case(dtype, H, dv, spread)
    assert 0 < ref["T"] <= SR.T_MAX[np.dtype(dtype)], (dtype, H, dv, spread, ref["T"])
    out = D.gatv2_replay(rp, ci, XT, XS, a, G2.SLOPE, D.DROP, D.SEED, None, dO)
    r = D.ratios(_got(out, GATV2_KEYS), ref)
    print("GATv2 replay under dropout on the chunk pattern, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s"
          % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_of_the_steep_rows_and_of_the_second_block(dtype):
    rp, ci, val, el, er, V, dO, ref = D.gat_steep_case(dtype)
    r = D.ratios(_got(D.gat_replay(rp, ci, el, er, V, G.SLOPE, D.DROP, D.SEED, val, dO), GAT_KEYS), ref)
    print("GAT replay under dropout, steep rows with bias (%s): %s" % (dtype, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r
    rp, ci, val, XT, XS, a, dO, ref = D.gatv2_steep_case(dtype)
    r = D.ratios(_got(D.gatv2_replay(rp, ci, XT, XS, a, G2.SLOPE, D.DROP, D.SEED, val, dO), GATV2_KEYS), ref)
    print("GATv2 replay under dropout, steep rows with bias (%s): %s" % (dtype, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1, r
    rp, ci, el, er, V, ref = D.gat_second_block_case(dtype)
    r = D.ratios(_got(D.gat_replay(rp, ci, el, er, V, G.SLOPE, D.DROP, D.SEED), G.FWD_KEYS), ref)
    assert max(r.values()) <= 1, r


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_entry_off_by_four_bounds_is_caught(dtype):
    """every output of both layers, one entry with a nonzero bound moved by four bounds: the ratio passes 1"""
    H, dv = 3, G.widths(dtype)[3]
    spread = G.SPREADS[(3 + H) % 2]
    rp, ci, el, er, V, dO, ref = D.gat_case(dtype, H, dv, spread)
    out = D.gat_replay(rp, ci, el, er, V, G.SLOPE, D.DROP, D.SEED, None, dO)
    rp, ci, XT, XS, a, dO2, ref2 = D.gatv2_case(dtype, H, dv, spread)
    out2 = D.gatv2_replay(rp, ci, XT, XS, a, G2.SLOPE, D.DROP, D.SEED, None, dO2)
    for out, ref, keys in ((out, ref, GAT_KEYS), (out2, ref2, GATV2_KEYS)):
        assert max(D.ratios(_got(out, keys), ref).values()) <= 1
        for k in keys:
            want, bnd = ref[k]
            live = np.flatnonzero((bnd.ravel() > 0) & np.isfinite(want.ravel().astype(np.float64)))
            at = live[live.size // 2]
            bad = out[k].copy()
            step = 4 * float(bnd.ravel()[at])
            moved = bad.ravel()[at] + bad.dtype.type(step)
            assert abs(float(moved) - float(bad.ravel()[at])) >= 3 * float(bnd.ravel()[at]), (k, "the bound is below the dtype's spacing")
            bad.reshape(-1)[at] = moved
            assert D.ratios({k: bad}, ref)[k] > 1, (dtype, k)


def test_a_wholly_dropped_row_has_zero_output_and_a_finite_lse():
    rp, ci, el, er, V, dO, ref = D.gat_case("float64", 3, 5, G.SPREADS[(1 + 3) % 2])
    out = D.gat_replay(rp, ci, el, er, V, G.SLOPE, D.DROP, D.SEED, None, dO)
    row, h = 8, 1
    assert not ref["k"][rp[row]:rp[row + 1], h].any()
    assert (out["O"][row, h * 5:(h + 1) * 5] == 0).all() and np.isfinite(out["lse"][row, h])
    assert (ref["O"][0][row, h * 5:(h + 1) * 5] == 0).all() and out["delta"][row, h] == 0 and np.isfinite(out["d_el"][row, h])
    assert (out["ds"][rp[row]:rp[row + 1], h] == 0).all()      # dP' = 0 and D = 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_product_with_rs_is_a_rounding_of_its_own(dtype):
    """fl(fl(dP rs) - D) differs from the contracted fma(dP, rs, -D) on the inexact data: the pins of the GPU tests can tell a
    kernel that contracts the two from one that does not.  rs = 1 / (1 - 0.6) is inexact in both dtypes."""
    dt = np.dtype(dtype)
    rp, ci, el, er, V, dO, _ = G.case(dtype, 1, 5, G.SPREADS[(1 + 1) % 2])
    rs = D.rs_of(0.6, dt)
    rows = np.repeat(np.arange(G.NROW), np.diff(rp))
    dP = np.einsum("ij,ij->i", dO[rows], V[ci]).astype(dt)
    Dl = np.random.default_rng(4).standard_normal(ci.size).astype(dt)
    two = ((dP * rs).astype(dt) - Dl).astype(dt)
    one = SR.fma(dP, np.full_like(dP, rs), -Dl)
    assert (two != one).any() and np.abs(two - one).max() <= 4 * D.U[dt] * np.abs(two).max()
