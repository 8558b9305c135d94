"""CPU: the fixed order of the fused GAT attention (csrc/gat_kernels.hip), replayed in numpy (tests/gat_ref.replay), meets the bound
of DESIGN.md 5o on the inputs of tests/test_gpu_gat.py, forward and backward, and the bound is tight enough to catch an entry that
is off by four bounds."""
import numpy as np
import pytest

import gat_ref as G
import softmax_ref as SR

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


def test_the_chunk_matrix_has_the_lengths_the_tests_rely_on():
    G.check_chunk_matrix()


def _census(dtype, kind, have):
    """the widths `have` reach every (LPR, P) of kind's dispatch table, both sides of every threshold, the last width of the table,
    the 16-byte and the element path of every instance, and an element-path width strictly inside the 32- and the 64-lane range"""
    w = G.W[dtype]
    fwd = kind == "gat_fwd"
    tops = [t * w for t, _ in G.INSTANCES]
    want = [inst for _, inst in G.INSTANCES] + ([(64, 8)] if fwd else [])
    by = {inst: [dv for dv in have if G.instance_of(kind, dtype, dv) == inst] for inst in want}
    assert sum(len(v) for v in by.values()) == len(have), (dtype, kind, "a width outside the table")
    for inst, dvs in by.items():
        assert any(dv % w == 0 for dv in dvs) and any(dv % w for dv in dvs), (dtype, kind, inst, dvs, "needs a 16-byte and an element width")
    for t in tops[:-1] + (tops[-1:] if fwd else []):
        assert t in have and t + 1 in have, (dtype, kind, t, "both sides of the threshold")
        assert G.instance_of(kind, dtype, t) != G.instance_of(kind, dtype, t + 1)
    assert tops[-1] in have, (dtype, kind, "P = 4, every piece full")
    if fwd:
        assert G.FWD_BLOCK * w in have and G.second_block_width(dtype) in have, (dtype, "P = 8 in one V block, full, and in two")
    for lo, hi in ((16 * w, 32 * w), (32 * w, 64 * w)):
        assert any(lo + 1 < dv < hi and dv % w for dv in have), (dtype, kind, lo, hi, "an element-path width inside the range")


def test_the_instances_are_the_ones_meant():
    """gat_ref.instance_of restates the three dispatch tables; widths() and chunk_widths() together reach every instance of every
    table on both sides of every threshold -- and no width of chunk_widths() can be left out"""
    assert G.instance_of("gat_fwd", "float64", 512) == (64, 4) and G.instance_of("gat_fwd", "float64", 513) == (64, 8)
    assert G.instance_of("gat_fwd", "float32", 1025) == (64, 8) and G.instance_of("gat_bwd", "float64", 17) == (16, 1)
    assert [G.instance_of("gatv2", "float32", dv) for dv in (32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == \
        [(8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 2), (64, 2), (64, 4), (64, 4)]
    with pytest.raises(AssertionError):
        G.instance_of("gat_bwd", "float64", 513)
    for dtype in DTYPES:
        for kind in G.KINDS:
            base = set(G.widths(dtype)) | ({G.second_block_width(dtype)} if kind == "gat_fwd" else set())
            chunk = G.chunk_widths(dtype, kind)
            assert len(set(chunk)) == len(chunk) and not base & set(chunk)
            _census(dtype, kind, base | set(chunk))
            for dv in chunk:
                with pytest.raises(AssertionError):
                    _census(dtype, kind, base | (set(chunk) - {dv}))


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


@pytest.mark.parametrize("dtype,H,dv,spread,backward", list(G.chunk_bound_cases()))
def test_replay_is_inside_the_bound_on_the_chunk_pattern(dtype, H, dv, spread, backward):
    """rows of up to 200 entries and a hub column of 277: 5j's data rule on the reference alone, then the replay against the bound"""
    rp, ci, el, er, V, dO, ref = G.chunk_case(dtype, H, dv, spread, backward)
    assert 0 < ref["T"] <= SR.T_MAX[np.dtype(dtype)], (dtype, H, dv, spread, ref["T"])
    out = G.replay(rp, ci, el, er, V, G.SLOPE, None, dO)
    r = G.ratios(_got(out, G.FWD_KEYS + (G.BWD_KEYS if backward else ())), ref)
    print("replay on the chunk pattern, worst |err| / bound (%s, H = %d, dv = %d, spread %g): %s"
          % (dtype, H, dv, spread, {k: "%.3g" % v for k, v in r.items()}))
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
