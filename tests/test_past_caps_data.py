"""CPU: the data of tests/test_gpu_past_caps.py (tests/past_caps.py).  Every shape is past the threshold it is meant for and its
small companion is not; the host C paths (hip.csr_transpose, partition.permute_sym on numpy arrays) equal the numpy definitions
on the valid shapes, which pins the references before a GPU sees them; the softmax replay lies inside the longdouble bounds;
and one negative control per family: a result in which the second trip's rows, columns or tiles keep their initial values
fails the comparison, so the data would notice a dropped trip.

Host paths left out here because they take too long on a CPU: none.  (Measured on a CPU-only machine: host transpose of the
16.8 M-nonzero matrix 2.5 s, its sort-based reference 1.2 s; the softmax replays 0.1 .. 2.2 s per case.)"""
import numpy as np
import pytest

import past_caps as P
import softmax_ref as R
from test_graph_part import numpy_permute
from test_transpose import numpy_transpose

NAMES = ("rowptr_t", "colidx_t", "val_t", "tmap")


def _same(want, got, tag):
    for k, (w, g) in enumerate(zip(want, got)):
        assert w.dtype == g.dtype and w.shape == g.shape and np.array_equal(w, g), (tag, k)


# ---- the thresholds themselves

def test_constants_mirror_the_sources():
    """the constants against the text of the launchers: a changed cap makes this file's shapes meaningless"""
    import os
    from conftest import ROOT
    src = lambda f: open(os.path.join(ROOT, "crp-spmm_amd", "csrc", f)).read()      # noqa: E731
    scan, tr, pm, sm, api, rk = (src(f) for f in ("scan_sort.h", "transpose_kernels.hip", "permute_kernels.hip", "softmax_kernels.hip",
                                                  "hip_api.hip", "row_kernels.hip"))
    assert "SCAN_THREADS = 256, SCAN_ITEMS = 8" in scan and "b0 += 1024" in scan and "LDS_PAIRS = 4096" in scan
    assert tr.count("1 << 16") == 2 and tr.count("1 << 20") == 2 and pm.count("1 << 16") == 1 and pm.count("1 << 20") == 1
    for text in (tr, pm):
        assert "(long long) 256 << 20" in text and "(long long) cs.n_long, 256, budget / (slice * 8)" in text
    assert "((int64_t) nrow + 3) / 4, 2048)" in sm
    assert "((long long) nrow + 3) / 4, 65536)" in api and "((long long) nrow + 3) / 4, 65536)" in rk
    assert "(words + 255) / 256, 1024)" in rk
    assert P.SCAN_CHUNK == 2097152 and P.PASS1_CAP == 16777216 and P.WAVE_ROWS_CAP == 4194304 and P.LONG_FULL_GRID_MAX == 131072
    assert P.GATHER_CAP == 262144 and P.COUNT_COLS_CAP == 8388608
    assert [P.sm_rows_per_trip(l) for l in (64, 32, 16, 8)] == [8192, 16384, 32768, 65536]
    from crp_spmm_amd import partition
    assert partition.PERMUTE_LDS_PAIRS == P.LDS_PAIRS


# ---- 1. the scan

def test_scan_shapes_and_the_model():
    assert [P.scan_tiles(n + 1) for n in P.SCAN_LARGE_NCOL] == [1024, 1025, 1028]
    assert [P.scan_trips(n + 1) for n in P.SCAN_LARGE_NCOL] == [1, 2, 2]                 # the companion, then two past the chunk
    assert P.SCAN_LARGE_NCOL[0] + 1 <= P.SCAN_CHUNK < P.SCAN_LARGE_NCOL[1] + 1
    assert [n % P.SCAN_TILE for n in P.SCAN_SMALL_N] == [2047, 0, 1, 0, 1]
    for ncol in P.SCAN_NCOLS:
        rp, ci, va, _ = P.scan_case(ncol)
        counts = np.bincount(ci, minlength=ncol)
        tile_has = np.add.reduceat(counts, np.arange(0, ncol, P.SCAN_TILE)) > 0
        assert tile_has.all(), ncol                                                       # every tile holds a non-empty column
        assert counts[0] > 0 and counts[ncol - 1] > 0
        x = np.concatenate([counts, [0]])
        want = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        assert np.array_equal(P.scan_model(x), want), ncol
        # the negative control: without the carry the later chunks start from zero again
        assert np.array_equal(P.scan_model(x, carry=False), want) == (P.scan_trips(ncol + 1) == 1), ncol
        # unsorted columns inside rows, duplicate pairs
        rows = R.rows_of(rp)
        assert (np.diff(ci.astype(np.int64))[np.diff(rows) == 0] < 0).any()
        pair = rows.astype(np.int64) * ncol + ci
        assert np.unique(pair).size <= pair.size - 400


@pytest.mark.parametrize("ncol", P.SCAN_NCOLS)
def test_scan_cases_host_transpose_equals_numpy(crp, ncol):
    from crp_spmm_amd import hip
    rp, ci, va, _ = P.scan_case(ncol)
    want = numpy_transpose(rp, ci, va, ncol)
    _same(want, hip.csr_transpose(rp, ci, va, ncol), ncol)
    _same(want, P.sort_transpose(rp, ci, va, ncol), (ncol, "the sort-based reference"))


# ---- 2. the transpose past its grid caps

def test_big_square_is_past_the_caps_and_its_host_transpose_equals_the_reference(crp):
    """Reference (sort_transpose) 1.2 s, host path 2.5 s on a CPU-only machine."""
    from crp_spmm_amd import hip
    rp, ci, va, n = P.big_square()
    nnz = ci.size
    assert n > P.WAVE_ROWS_CAP and nnz > P.PASS1_CAP and nnz == rp[-1]
    counts = np.bincount(ci, minlength=n)
    assert P.WAVE < counts[P.BIG_MID_COL] <= P.LDS_PAIRS < counts[P.BIG_LONG_COL]
    assert min(P.BIG_MID_COL, P.BIG_LONG_COL) > P.WAVE_ROWS_CAP
    assert (counts[P.WAVE_ROWS_CAP:] > 0).sum() > 5000                                   # columns past the cap hold nonzeros
    want = P.sort_transpose(rp, ci, va, n)
    _same(want, hip.csr_transpose(rp, ci, va, n), "big")
    # the sort-based reference is numpy_transpose: on a slice of rows small enough for the stable argsort
    k = 300000
    _same(numpy_transpose(rp[:k + 1], ci[:4 * k], va[:4 * k], n), P.sort_transpose(rp[:k + 1], ci[:4 * k], va[:4 * k], n), "slice")
    # negative controls: the nonzeros past the pass-1 cap change the counts; the rows past the wave cap own output entries
    assert not np.array_equal(np.bincount(ci[:P.PASS1_CAP], minlength=n), counts)
    assert (want[1] >= P.WAVE_ROWS_CAP).sum() == 4 * (n - P.WAVE_ROWS_CAP)
    assert (np.diff(want[0])[P.WAVE_ROWS_CAP:] > 0).all() or (np.diff(want[0])[P.WAVE_ROWS_CAP:] > 0).sum() > 5000
    # unsorted rows and duplicate pairs
    quad = ci.reshape(n, 4).astype(np.int64)
    assert (quad[:, 0] > quad[:, 1]).sum() > n // 2 and (quad[:, 2] == quad[:, 3]).sum() > 4000


def test_tall_wide_is_past_the_caps_and_its_host_transpose_equals_numpy(crp):
    from crp_spmm_amd import hip
    rp, ci, va, ncol = P.tall_wide()
    nrow = rp.size - 1
    assert nrow > P.PASS1_CAP and ncol > P.PASS1_CAP and 90000 < ci.size < 150000
    counts = np.bincount(ci, minlength=ncol)
    assert P.WAVE < counts[P.TALL_MID_COL] <= P.LDS_PAIRS < counts[P.TALL_LONG_COL]
    assert min(P.TALL_MID_COL, P.TALL_LONG_COL) > P.PASS1_CAP
    lens = np.diff(rp)
    for r in (0, P.WAVE_ROWS_CAP - 1, P.WAVE_ROWS_CAP, P.PASS1_CAP - 1, P.PASS1_CAP, nrow - 1):
        assert lens[r] > 0, r
    assert lens[P.PASS1_CAP:].sum() > 3000
    want = numpy_transpose(rp, ci, va, ncol)
    _same(want, hip.csr_transpose(rp, ci, va, ncol), "tall")
    # negative controls: the tiers past the cap, the rows past the cap
    assert not np.array_equal(np.bincount(ci[:rp[P.PASS1_CAP]], minlength=ncol), counts)
    assert (counts[P.PASS1_CAP:] > P.WAVE).sum() == 2 and (want[1] >= P.PASS1_CAP).sum() == lens[P.PASS1_CAP:].sum()


@pytest.mark.parametrize("which", P.LONG_CASES)
def test_long_queue_shapes(crp, which):
    from crp_spmm_amd import hip, partition
    rp, ci, va, ncol = P.long_columns(which)
    prp, pci, pva, perm = P.long_rows(which)
    for lens in (np.bincount(ci, minlength=ncol), np.diff(prp)):
        n_long, max_long = P.long_census(lens)
        grid, slice_ = P.long_grid(n_long, max_long)
        if which == "many":
            assert n_long == 300 > P.LONG_GRID == grid and slice_ == 16384 and max_long <= P.LONG_FULL_GRID_MAX
            longs = lens[lens > P.LDS_PAIRS]
            assert {8191, 8192, 8193} <= set(longs.tolist()) and (longs <= 8192).sum() > 50 and (longs > 8192).sum() > 20
        else:
            assert max_long >= 140000 > P.LONG_FULL_GRID_MAX and slice_ == 262144 and grid == 128 < n_long == 201
        # the negative control: workgroups that sort one row each leave n_long - grid rows of the queue unsorted
        assert n_long - grid >= 44
        # and the companion below the thresholds: the tier matrix of the older tests (3 long rows, one trip, the full grid)
        assert P.long_grid(3, 70001) == (3, 131072)
    want = numpy_transpose(rp, ci, va, ncol)
    _same(want, hip.csr_transpose(rp, ci, va, ncol), which)
    assert not np.array_equal(want[3], np.sort(want[3]))                                  # the fill order is not the answer
    _same(numpy_permute(prp, pci, pva, perm), partition.permute_sym(prp, pci, pva, perm), which)


# ---- 3. the permutation

def test_tall_square_is_past_the_caps_and_its_host_permutation_equals_numpy(crp):
    from crp_spmm_amd import partition
    rp, ci, va, perm = P.tall_square()
    n = rp.size - 1
    assert n > P.PASS1_CAP and 150000 < ci.size < 250000 and P.scan_trips(n + 1) == 9
    lens = np.diff(rp)
    for r in (0, P.WAVE_ROWS_CAP - 1, P.WAVE_ROWS_CAP, P.PASS1_CAP - 1, P.PASS1_CAP, n - 1):
        assert lens[r] > 0, r
    mid, long_ = np.flatnonzero((lens > P.WAVE) & (lens <= P.LDS_PAIRS)), np.flatnonzero(lens > P.LDS_PAIRS)
    assert mid.size == 2 and long_.size == 1 and mid.min() > P.WAVE_ROWS_CAP and long_[0] > P.WAVE_ROWS_CAP and mid.max() > P.PASS1_CAP
    assert np.array_equal(np.sort(perm), np.arange(n))
    want = numpy_permute(rp, ci, va, perm)
    _same(want, partition.permute_sym(rp, ci, va, perm), "tall_square")
    # negative controls: rows past either cap own entries of the output; without the scan's carry the row pointer differs
    len1 = np.diff(want[0])
    assert np.array_equal(len1[perm], lens)
    assert not np.array_equal(P.scan_model(np.concatenate([len1, [0]]), carry=False), want[0])
    dropped = lens.copy()
    dropped[P.PASS1_CAP:] = 0
    assert not np.array_equal(dropped, lens) and lens[P.WAVE_ROWS_CAP:].sum() > 10000


# ---- 4. the softmax

@pytest.mark.parametrize("lpr", P.SM_LPRS)
def test_softmax_shapes(lpr):
    rp = P.sm_rowptr(lpr)
    nrow, trip, rpb = rp.size - 1, P.sm_rows_per_trip(lpr), 256 // lpr
    assert R.lpr_of(rp) == lpr
    assert nrow > 3 * trip and nrow % rpb != 0 and (nrow + 3) // 4 > P.SM_GRID
    assert 900000 < rp[-1] < 2000000
    lens = np.diff(rp)
    for t in range(4):                                                        # both row paths and empty rows in every trip
        part = lens[t * trip:(t + 1) * trip]
        assert (part == 0).any() and ((part > 0) & (part <= 8 * lpr)).any() and (part > 8 * lpr).any(), (lpr, t)
    special = P.sm_special_rows(lpr)
    for (r0, r1), t in zip(P.sm_windows(lpr), (1, 2)):
        assert t * trip <= r0 < r1 <= (t + 1) * trip
        inside = [r for r in special if r0 <= r < r1]
        assert len(inside) == 10 and all(lens[r] == special[r][0] for r in inside)
    # the companions below the cap: the row pointers of tests/test_gpu_row_softmax.py
    for name in R.PATTERNS + R.EDGE_PATTERNS:
        small = R.pattern(name)
        assert small.size - 1 <= P.sm_rows_per_trip(R.lpr_of(small)), name


@pytest.mark.parametrize("lpr", P.SM_LPRS)
@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_softmax_replay_inside_the_bounds(dtype, lpr):
    rp, s, ref, bound, y, dy, ref_b, bound_b = P.sm_case(lpr, dtype)
    trip = P.sm_rows_per_trip(lpr)
    w, at = R.worst(y, ref, bound)
    assert w <= 1.0, (lpr, "forward", w, at)
    gb = R.replay_bwd(rp, y, dy)
    w, at = R.worst(gb, ref_b, bound_b)
    assert w <= 1.0, (lpr, "backward", w, at)
    for r, (length, masked) in P.sm_special_rows(lpr).items():
        row = y[rp[r]:rp[r + 1]]
        assert row.size == length and (not masked or (row == 0).all()) and (length != 1 or row[0] == 1)
    # the negative control: the rows of the later trips left at NaN miss the bound
    for got, rf, bd in ((y, ref, bound), (gb, ref_b, bound_b)):
        dropped = np.array(got)
        dropped[rp[trip]:] = np.nan
        assert rp[trip] < rp[-1] and not R.worst(dropped, rf, bd)[0] <= 1.0


# ---- 5. the gather and the comm-size kernels

def test_gather_shape():
    full_rp, rows, sub_rp, sub_ci, start = P.gather_case()
    assert rows.size == P.GATHER_SUB_ROWS > P.GATHER_CAP and (np.diff(rows) > 0).all() and rows.size < full_rp.size - 1
    lens = np.diff(sub_rp)
    assert 2.5 < lens.mean() < 3.5 and (lens[P.GATHER_CAP:] > 0).sum() > 3000 and (lens > 64).sum() >= 150
    assert (lens[P.GATHER_CAP:] > 64).any()
    idx = P.gather_index(full_rp, rows, sub_rp)
    assert np.array_equal(idx[sub_rp[:-1][lens > 0]], start[lens > 0]) and (np.diff(idx) > 0).all() and idx[-1] < full_rp[-1]
    assert np.array_equal(start, full_rp[rows])
    # the negative control: a gather that stops at the cap leaves the later rows' values as they were
    full_val = np.random.default_rng(1).standard_normal(int(full_rp[-1]))
    got = np.zeros(idx.size)
    got[:sub_rp[P.GATHER_CAP]] = full_val[idx[:sub_rp[P.GATHER_CAP]]]
    assert not np.array_equal(got, full_val[idx])
    # the companion: tests/test_gpu_parity.py::test_create_with_device_values gathers 2000 rows
    assert 2000 <= P.GATHER_CAP


def test_comm_shape_and_host_planner_equals_oracle(crp, orc):
    from crp_spmm_amd import planner
    rp, ci, va, ncol = P.comm_case()
    nrow = rp.size - 1
    assert nrow > P.GATHER_CAP and ncol > P.COUNT_COLS_CAP and (ncol + 31) // 32 > P.COUNT_WORDS_CAP
    assert 20011 <= P.GATHER_CAP and 20011 <= P.COUNT_COLS_CAP                            # the largest shape of the older test
    word = ci >> 5
    assert (word < P.COUNT_WORDS_CAP).sum() > 1000 and (word >= P.COUNT_WORDS_CAP).sum() > 1000
    assert {P.COUNT_WORDS_CAP - 1, P.COUNT_WORDS_CAP} <= set(word.tolist())
    tags = []
    for tag, rb, xd in P.comm_partitions(planner, rp, nrow, ncol):
        tags.append(tag)
        sizes, tot = planner.csr_mat_row_part_comm_size(ncol, rp, ci, rb, xd)
        o_sizes, o_tot = orc.csr_row_part_comm_size(ncol, rp, ci, rb, xd)
        assert np.array_equal(np.asarray(o_sizes), sizes) and int(o_tot) == tot, tag
        assert (tot > 0) == (tag != "P=1"), tag                                            # (one block owns every column)
        if tot == 0:
            continue
        # negative controls: the rows past the mark kernel's cap, and the columns past the count kernel's, change the sizes
        cut = rp.copy()
        cut[P.GATHER_CAP + 1:] = cut[P.GATHER_CAP]
        rows_cut, _ = planner.csr_mat_row_part_comm_size(ncol, cut, ci, rb, xd)
        assert not np.array_equal(rows_cut, sizes), tag
        outside = sum(np.unique(c[(c < xd[b]) | (c >= xd[b + 1])]).size
                      for b in range(rb.size - 1) for c in [ci[rp[rb[b]]:rp[rb[b + 1]]]])
        assert outside == tot, tag                                                         # the definition, in numpy
        low = sum(np.unique(c[((c < xd[b]) | (c >= xd[b + 1])) & (c < P.COUNT_COLS_CAP)]).size
                  for b in range(rb.size - 1) for c in [ci[rp[rb[b]]:rp[rb[b + 1]]]])
        assert low < tot, tag
    assert tags == ["P=1", "P=3", "P=8", "ragged"]
