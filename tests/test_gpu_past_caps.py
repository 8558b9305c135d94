"""GPU: the device kernels past their grid caps and chunk limits, on the shapes of tests/past_caps.py (whose data
tests/test_past_caps_data.py checks on the CPU): the second and later trips of every capped grid-stride loop, the carry of the
scan's later chunks and the second row in a scratch slice of the long-row queue run under bitwise checks against numpy.

  1  the scan of csrc/scan_sort.h through crp_csr_transpose: ncol + 1 on the tile edges and 1024 / 1025 / 1028 tiles
  2  the transpose past the caps of k_check_count, k_tiers, k_fill_keys, k_sort_short; refusals found past the cap; k_sort_long
     with more long rows than workgroups and with a budget-limited grid
  3  the permutation P A P^T past the same caps
  4  the row softmax past sm_grid, for every lane group, both dtypes, forward and backward
  5  the gather of crp_csr_dev_create_dv and the planner's comm-size kernels

Every test asserts that its shape is past its threshold; the companions below the thresholds are the shapes of the older tests
(tests/test_past_caps_data.py names them).  Every test prints its wall time on the device."""
import ctypes as C
import time

import numpy as np
import pytest

import past_caps as P
import softmax_ref as R
from test_graph_part import numpy_permute
from test_transpose import numpy_transpose

pytestmark = pytest.mark.gpu

SENT = -77
NAMES = ("rowptr_t", "colidx_t", "val_t", "tmap")


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.array(a, order="C")).to(gpu) for a in arrays]


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(want, got, tag):
    for k, (w, g) in enumerate(zip(want, got)):
        assert w.dtype == g.dtype and w.shape == g.shape and np.array_equal(w, g), (tag, k)


def _device_transpose(gpu, rp, ci, va, ncol, tag):
    import torch
    from crp_spmm_amd import hip
    args = _dev(gpu, rp, ci, va)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = hip.csr_transpose(*args, ncol)
    torch.cuda.synchronize()
    print("%s: device transpose %.3f s" % (tag, time.perf_counter() - t0))
    return [t.cpu().numpy() for t in got]


def _device_permute(gpu, rp, ci, va, perm, tag):
    import torch
    from crp_spmm_amd import partition
    args = _dev(gpu, rp, ci, va, perm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = partition.permute_sym(*args)
    torch.cuda.synchronize()
    print("%s: device permutation %.3f s" % (tag, time.perf_counter() - t0))
    return [t.cpu().numpy() for t in got]


# ---- 1. the scan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncol", P.SCAN_NCOLS)
def test_scan_tile_edges_and_chunks_through_the_transpose(crp, gpu, ncol):
    """ncol + 1 counts: one tile less one, one tile, one more, two tiles, one more; 1024 tiles (the companion: one trip over the
    tile sums, no carry), 1025 and 1028 tiles (a second trip, whose offsets start from the first chunk's total)."""
    from crp_spmm_amd import hip
    if ncol == P.SCAN_LARGE_NCOL[0]:
        assert P.scan_trips(ncol + 1) == 1 and ncol + 1 == P.SCAN_CHUNK
    elif ncol > P.SCAN_LARGE_NCOL[0]:
        assert P.scan_trips(ncol + 1) == 2 and ncol + 1 > P.SCAN_CHUNK
    else:
        assert (ncol + 1) % P.SCAN_TILE in (P.SCAN_TILE - 1, 0, 1)
    rp, ci, va, _ = P.scan_case(ncol)
    got = _device_transpose(gpu, rp, ci, va, ncol, "scan %d" % ncol)
    _same(numpy_transpose(rp, ci, va, ncol), got, (ncol, "against numpy"))
    _same(hip.csr_transpose(rp, ci, va, ncol), got, (ncol, "against the host path"))


# ---- 2. the transpose ----------------------------------------------------------------------------------------------------

_cache = {}


def _big_want():
    if "big" not in _cache:
        t0 = time.perf_counter()
        _cache["big"] = P.sort_transpose(*P.big_square())
        print("big: reference %.2f s" % (time.perf_counter() - t0))
    return _cache["big"]


def _tall_want():
    if "tall" not in _cache:
        _cache["tall"] = numpy_transpose(*P.tall_wide())
    return _cache["tall"]


def _tall_square_want():
    if "tall_square" not in _cache:
        _cache["tall_square"] = numpy_permute(*P.tall_square())
    return _cache["tall_square"]


def test_transpose_past_the_nonzero_and_wave_caps(crp, gpu):
    """4 200 000 rows and columns, 16 800 000 nonzeros: the second trip of k_check_count's nonzero branch, of k_fill_keys and of
    k_sort_short, and a three-chunk scan, in one call.  The reference is one np.sort of (column << 32 | position) and the gathers
    that follow it: 1.2 s measured on a CPU-only machine (generating the matrix: 0.5 s)."""
    rp, ci, va, n = P.big_square()
    assert n > P.WAVE_ROWS_CAP and ci.size > P.PASS1_CAP and P.scan_trips(n + 1) == 3
    want = _big_want()
    counts = np.diff(want[0])
    assert P.WAVE < counts[P.BIG_MID_COL] <= P.LDS_PAIRS < counts[P.BIG_LONG_COL] and P.BIG_MID_COL > P.WAVE_ROWS_CAP
    _same(want, _device_transpose(gpu, rp, ci, va, n, "big"), "big")


def test_transpose_past_the_row_and_tier_caps(crp, gpu):
    """16 778 216 rows (k_check_count's row branch; k_fill_keys four times over) and 16 778 716 columns with a mid-tier and a long
    column past column 16 777 216 (k_tiers, k_sort_short), about 10^5 nonzeros; a nine-chunk scan."""
    rp, ci, va, ncol = P.tall_wide()
    assert rp.size - 1 > P.PASS1_CAP and ncol > P.PASS1_CAP and P.scan_trips(ncol + 1) == 9
    want = _tall_want()
    counts = np.diff(want[0])
    assert P.WAVE < counts[P.TALL_MID_COL] <= P.LDS_PAIRS < counts[P.TALL_LONG_COL] and P.TALL_MID_COL > P.PASS1_CAP
    _same(want, _device_transpose(gpu, rp, ci, va, ncol, "tall"), "tall")


def _raw_transpose(lib, gpu, d_rp, d_ci, d_va, ncol):
    """(code, nothing but rowptr_t written) of a raw call into outputs that hold a sentinel"""
    import torch
    nnz = d_ci.numel()
    rp_t = torch.full((ncol + 1,), SENT, dtype=torch.int32, device=gpu)
    ci_t = torch.full((nnz,), SENT, dtype=torch.int32, device=gpu)
    va_t = torch.full((nnz,), float(SENT), dtype=torch.float64, device=gpu)
    tmap = torch.full((nnz,), SENT, dtype=torch.int32, device=gpu)
    rc = lib.crp_csr_transpose(d_rp.numel() - 1, ncol, C.c_void_p(d_rp.data_ptr()), C.c_void_p(d_ci.data_ptr()), C.c_void_p(d_va.data_ptr()),
                               C.c_void_p(rp_t.data_ptr()), C.c_void_p(ci_t.data_ptr()), C.c_void_p(va_t.data_ptr()),
                               C.c_void_p(tmap.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, bool((ci_t == SENT).all()) and bool((va_t == SENT).all()) and bool((tmap == SENT).all())


def _first_empty_row(rp, r):
    lens = np.diff(rp)
    r += int(np.argmax(lens[r:] == 0))
    assert lens[r] == 0 and rp[r] + 1 <= rp[-1]
    return r


def test_transpose_refuses_what_only_a_later_trip_sees(crp, gpu):
    """A bad column at a position past 16 777 216, a row pointer that decreases at a row past 16 777 216: codes, nothing written but
    rowptr_t, and the valid call afterwards still matches.  (Pass 1 reads colidx inside [0, nnz) and rowptr inside [0, nrow] only,
    and indexes the counts with a column only after the range check.)"""
    import torch
    from crp_spmm_amd import _lib, hip
    lib = _lib.load()
    rp, ci, va, n = P.big_square()
    d_rp, d_ci, d_va = _dev(gpu, rp, ci, va)
    pos = P.PASS1_CAP + 12345
    assert P.PASS1_CAP < pos < ci.size
    t0 = time.perf_counter()
    for bad in (n, ~5):
        d_bad = d_ci.clone()
        d_bad[pos] = bad
        assert _raw_transpose(lib, gpu, d_rp, d_bad, d_va, n) == (hip.T_ECOL, True), bad
        del d_bad
    got = hip.csr_transpose(d_rp, d_ci, d_va, n)
    _same(_big_want(), [_host(t) for t in got], "big, after an error")
    del got, d_rp, d_ci, d_va
    rp, ci, va, ncol = P.tall_wide()
    r = _first_empty_row(rp, P.PASS1_CAP + 500)
    assert r > P.PASS1_CAP
    d_rp, d_ci, d_va = _dev(gpu, rp, ci, va)
    d_bad = d_rp.clone()
    d_bad[r] += 1                                                             # rowptr[r + 1] < rowptr[r]; rowptr[nrow] as before
    assert _raw_transpose(lib, gpu, d_bad, d_ci, d_va, ncol) == (hip.T_EPTR, True)
    got = hip.csr_transpose(d_rp, d_ci, d_va, ncol)
    _same(_tall_want(), [_host(t) for t in got], "tall, after an error")
    torch.cuda.synchronize()
    print("transpose refusals: %.3f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("which", P.LONG_CASES)
def test_transpose_long_row_queue(crp, gpu, which):
    """many: 300 long output rows for 256 workgroups -- 44 slices take a second row, and rows padded to 8192 and to 16 384 keys
    meet in one 16 384-key slice.  budget: a 140 000-entry row makes the slice 262 144 keys, the budget allows 128 workgroups for
    201 long rows."""
    rp, ci, va, ncol = P.long_columns(which)
    n_long, max_long = P.long_census(np.bincount(ci, minlength=ncol))
    grid, slice_ = P.long_grid(n_long, max_long)
    if which == "many":
        assert n_long > P.LONG_GRID == grid and slice_ == 16384
    else:
        assert max_long > P.LONG_FULL_GRID_MAX and grid == 128 < n_long
    _same(numpy_transpose(rp, ci, va, ncol), _device_transpose(gpu, rp, ci, va, ncol, "long " + which), which)


# ---- 3. the permutation --------------------------------------------------------------------------------------------------

def test_permutation_past_the_row_caps(crp, gpu):
    """16 780 217 rows, about 2 10^5 nonzeros on both sides of rows 4 194 304 and 16 777 216, a mid-tier and a long row past
    4 194 304, a random permutation: the later trips of k_scatter_lengths and k_sort_short and a nine-chunk scan."""
    from crp_spmm_amd import partition
    rp, ci, va, perm = P.tall_square()
    n = rp.size - 1
    assert n > P.PASS1_CAP > P.WAVE_ROWS_CAP and P.scan_trips(n + 1) == 9
    got = _device_permute(gpu, rp, ci, va, perm, "tall_square")
    _same(_tall_square_want(), got, "against numpy")
    _same(partition.permute_sym(rp, ci, va, perm), got, "against the host path")


def test_permutation_refuses_what_only_a_later_trip_sees(crp, gpu):
    import torch
    from crp_spmm_amd import partition
    rp, ci, va, perm = P.tall_square()
    n = rp.size - 1
    d_rp, d_ci, d_va, d_perm = _dev(gpu, rp, ci, va, perm)
    i = P.PASS1_CAP + 100
    assert P.PASS1_CAP < i < n - 1
    t0 = time.perf_counter()

    def code(*args):
        with pytest.raises(partition.PartitionError) as e:
            partition.permute_sym(*args)
        torch.cuda.synchronize()
        return e.value.code

    dup = d_perm.clone()
    dup[i] = dup[i + 1]                                                       # both hits of the target come from rows past the cap
    assert code(d_rp, d_ci, d_va, dup) == partition.EPERM
    out = d_perm.clone()
    out[i] = n + 5
    assert code(d_rp, d_ci, d_va, out) == partition.EPERM
    r = _first_empty_row(rp, P.PASS1_CAP + 500)
    bad = d_rp.clone()
    bad[r] += 1
    assert code(bad, d_ci, d_va, d_perm) == partition.EPTR
    del dup, out, bad
    # a column >= nrow at a position past the cap, in the matrix of 16 800 000 nonzeros
    brp, bci, bva, bn = P.big_square()
    pos = P.PASS1_CAP + 12345
    assert bci.size > pos > P.PASS1_CAP
    b_rp, b_ci, b_va = _dev(gpu, brp, bci, bva)
    b_perm = torch.randperm(bn, device=gpu).to(torch.int32)
    b_ci[pos] = bn
    assert code(b_rp, b_ci, b_va, b_perm) == partition.ECOL
    del b_rp, b_ci, b_va, b_perm
    # the valid call afterwards
    got = partition.permute_sym(d_rp, d_ci, d_va, d_perm)
    _same(_tall_square_want(), [_host(t) for t in got], "after the errors")
    print("permutation refusals: %.3f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("which", P.LONG_CASES)
def test_permutation_long_row_queue(crp, gpu, which):
    from crp_spmm_amd import partition
    rp, ci, va, perm = P.long_rows(which)
    n_long, max_long = P.long_census(np.diff(rp))
    grid, slice_ = P.long_grid(n_long, max_long)
    if which == "many":
        assert n_long > P.LONG_GRID == grid and slice_ == 16384
    else:
        assert max_long > P.LONG_FULL_GRID_MAX and grid == 128 < n_long
    got = _device_permute(gpu, rp, ci, va, perm, "long " + which)
    _same(numpy_permute(rp, ci, va, perm), got, which)
    _same(partition.permute_sym(rp, ci, va, perm), got, (which, "against the host path"))


# ---- 4. the row softmax --------------------------------------------------------------------------------------------------
DTYPES = ("f64", "f32")
G = 9                        # guard entries of NaN before the first row's entries and after the last row's


def _dt(dt):
    import torch
    return (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)


def _guard(a):
    pad = np.full(G, np.nan, a.dtype)
    return np.concatenate([pad, a, pad])


def _nan_like(gpu, n, tdt):
    import torch
    return torch.full((n,), float("nan"), dtype=tdt, device=gpu)


def _inside(full, nnz, tag):
    """the rows' part of a guarded result; the guards still NaN, no NaN inside"""
    assert np.isnan(full[:G]).all() and np.isnan(full[G + nnz:]).all(), (tag, "a guard was written")
    got = full[G:G + nnz]
    assert not np.isnan(got).any(), (tag, "NaN left inside the rows", int(np.isnan(got).sum()))
    return got


def _softmax_run(gpu, dt, lpr):
    """the guarded forward and backward results of the big call, and the device arrays"""
    from crp_spmm_amd import hip
    ndt, tdt = _dt(dt)
    rp, s, ref, bound, y, dy, ref_b, bound_b = P.sm_case(lpr, ndt)
    nrow, nnz = rp.size - 1, s.size
    assert R.lpr_of(rp) == lpr and nrow > 3 * P.sm_rows_per_trip(lpr) and nrow % (256 // lpr) != 0 and (nrow + 3) // 4 > P.SM_GRID
    dev = _dev(gpu, (rp + G).astype(np.int32), _guard(s), _guard(y), _guard(dy))
    t0 = time.perf_counter()
    fwd = _host(hip.row_softmax(dev[0], dev[1], out=_nan_like(gpu, nnz + 2 * G, tdt)))
    bwd = _host(hip.row_softmax_bwd(dev[0], dev[2], dev[3], out=_nan_like(gpu, nnz + 2 * G, tdt)))
    print("softmax %s LPR %d: %d rows, %d entries, forward + backward with downloads %.3f s" % (dt, lpr, nrow, nnz, time.perf_counter() - t0))
    return dev, fwd, bwd


@pytest.mark.parametrize("lpr", P.SM_LPRS)
@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_past_the_grid_cap(crp, gpu, dt, lpr):
    """More than three trips of the row loop, the last one partial: the whole result inside the derived bounds against
    np.longdouble; no NaN left of the pre-filled output inside the rows and the guards untouched; the special rows exactly; the
    windows of the second and of the third trip bit-identical to a small call on rowptr[r0 : r1 + 1]; the in-place forms."""
    from crp_spmm_amd import hip
    ndt, tdt = _dt(dt)
    rp, s, ref, bound, y, dy, ref_b, bound_b = P.sm_case(lpr, ndt)
    nnz = s.size
    (rg_d, sg_d, yg_d, dyg_d), fwd, bwd = _softmax_run(gpu, dt, lpr)
    got, gb = _inside(fwd, nnz, "forward"), _inside(bwd, nnz, "backward")
    w, at = R.worst(got, ref, bound)
    print("forward worst |err| / bound = %.3g at %d" % (w, at))
    assert w <= 1.0, ("forward bound missed", w, at)
    w, at = R.worst(gb, ref_b, bound_b)
    print("backward worst |err| / bound = %.3g at %d" % (w, at))
    assert w <= 1.0, ("backward bound missed", w, at)
    lens = np.diff(rp)
    assert (got[np.isneginf(s)] == 0).all() and (got[rp[:-1][lens == 1]] == 1).all()
    for r, (length, masked) in P.sm_special_rows(lpr).items():
        assert lens[r] == length and (not masked or (got[rp[r]:rp[r + 1]] == 0).all()), r
    # the rows of the later trips, from a call of their own
    trip = P.sm_rows_per_trip(lpr)
    for (r0, r1), t in zip(P.sm_windows(lpr), (1, 2)):
        assert t * trip <= r0 < r1 <= (t + 1) * trip
        lo, hi = int(rp[r0]) + G, int(rp[r1]) + G
        small = _host(hip.row_softmax(rg_d[r0:r1 + 1], sg_d, out=_nan_like(gpu, nnz + 2 * G, tdt)))
        assert np.array_equal(small[lo:hi], fwd[lo:hi]), (t, "forward")
        assert np.isnan(small[:lo]).all() and np.isnan(small[hi:]).all(), (t, "outside the window")
        small = _host(hip.row_softmax_bwd(rg_d[r0:r1 + 1], yg_d, dyg_d, out=_nan_like(gpu, nnz + 2 * G, tdt)))
        assert np.array_equal(small[lo:hi], bwd[lo:hi]), (t, "backward")
        assert np.isnan(small[:lo]).all() and np.isnan(small[hi:]).all(), (t, "backward, outside the window")
    # in place
    t = sg_d.clone()
    assert hip.row_softmax(rg_d, t, out=t) is t
    assert np.array_equal(_host(t), fwd, equal_nan=True), "y == s"
    t = dyg_d.clone()
    hip.row_softmax_bwd(rg_d, yg_d, t, out=t)
    assert np.array_equal(_host(t), bwd, equal_nan=True), "ds == dy"


def _replay_differences(what, dt, lpr, got, want, rp):
    diff = got != want
    rows = R.rows_of(rp)
    print("%s %s LPR %d: %d of %d entries differ from the replay, in %d rows; by trip %s" % (
        what, dt, lpr, int(diff.sum()), diff.size, np.unique(rows[diff]).size,
        np.bincount(rows[diff] // P.sm_rows_per_trip(lpr), minlength=4).tolist()))
    return int(diff.sum())


@pytest.mark.parametrize("lpr", P.SM_LPRS)
@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_backward_past_the_grid_cap_equals_the_replay(crp, gpu, dt, lpr):
    """The whole backward result of the same call, bit for bit, against softmax_ref.replay_bwd (all rows: 0.1 .. 2.2 s per case
    on a CPU, the 8-lane cases with their 197 611 rows the most).  The backward is FMAs, one subtraction and one product per
    entry, so the replay -- whose fma rounds once -- gives the device's bits."""
    ndt, _tdt = _dt(dt)
    rp, s, _ref, _bound, y, dy, _rb, _bb = P.sm_case(lpr, ndt)
    _dev_arrays, _fwd, bwd = _softmax_run(gpu, dt, lpr)
    assert _replay_differences("backward", dt, lpr, bwd[G:G + s.size], R.replay_bwd(rp, y, dy), rp) == 0


def _device_library_exp(gpu):
    """exp of a numpy array by the device library, through torch's elementwise kernel: none of the code under test"""
    import torch

    def exp(x):
        return torch.exp(torch.from_numpy(np.ascontiguousarray(x)).to(gpu)).cpu().numpy()
    return exp


@pytest.mark.parametrize("lpr", P.SM_LPRS)
@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_forward_past_the_grid_cap_equals_the_replay(crp, gpu, dt, lpr):
    """The whole forward result of the same call, bit for bit, against softmax_ref.replay_fwd (all rows: 0.1 .. 1.6 s per case on
    a CPU).  The replay takes its exponential from the device library (torch.exp on the device), as the kernel does: with
    numpy's exp the two differ in the last bit of 5 .. 42 % of the entries, the same share in each of the four trips of the row
    loop (f64 LPR 8: 53 165 of 959 418, by trip [17826, 17769, 17326, 244]; f32 LPR 64: 653 788 of 1 547 805, by trip [209899,
    208352, 210322, 25215]), which says nothing about a trip.  The maximum, the subtraction, the 64 strided partials, the tree
    and the division are numpy's, in the replay's order."""
    ndt, _tdt = _dt(dt)
    rp, s, _ref, _bound, y, _dy, _rb, _bb = P.sm_case(lpr, ndt)
    _dev_arrays, fwd, _bwd = _softmax_run(gpu, dt, lpr)
    got = fwd[G:G + s.size]
    _replay_differences("forward, numpy's exp", dt, lpr, got, y, rp)
    want = R.replay_fwd(rp, s, exp=_device_library_exp(gpu))
    assert _replay_differences("forward, the device library's exp", dt, lpr, got, want, rp) == 0


# ---- 5. the gather of create_dv and the comm-size kernels ------------------------------------------------------------------

def test_create_dv_gathers_past_the_grid_cap(crp, orc, gpu):
    """269 147 rows gathered from a 300 000-row matrix's values in device memory, one wave per row over 65 536 x 4 waves: the
    product of the handle at width 8 through the CSR kernel (which reads the handle's device values) on exact data equals
    C_exact bit for bit, so every gathered value is in its place."""
    import torch
    import fp64_ref
    lib = crp.load()
    _IP, _DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    full_rp, rows, sub_rp, sub_ci, start = P.gather_case()
    m, k, n = rows.size, P.GATHER_NCOL, 8
    lens = np.diff(sub_rp)
    assert m > P.GATHER_CAP and (lens[P.GATHER_CAP:] > 64).any() and lens[P.GATHER_CAP:].sum() > 3000
    val, B, C_exact = fp64_ref.exact_problem(sub_rp, sub_ci, k, n, np.random.default_rng(5), "A")
    full_val = np.full(int(full_rp[-1]), 7.0)                                 # the rows that are not gathered hold sevens
    full_val[P.gather_index(full_rp, rows, sub_rp)] = val
    sub_rp, sub_ci, val = (np.ascontiguousarray(a) for a in (sub_rp, sub_ci, val))
    va_dev, Bd = _dev(gpu, full_val, B)
    h = C.c_void_p()
    t0 = time.perf_counter()
    assert lib.crp_csr_dev_create_dv(m, k, sub_rp.ctypes.data_as(_IP), sub_ci.ctypes.data_as(_IP), val.ctypes.data_as(_DP),
                                     C.c_void_p(va_dev.data_ptr()), start.ctypes.data_as(_IP), C.byref(h)) == 0
    Cd = torch.full((m, n), float("nan"), dtype=torch.float64, device=gpu)
    assert lib.crp_spmm_csr_f64(h, 0, n, C.c_void_p(Bd.data_ptr()), n, None, 0, C.c_void_p(Cd.data_ptr()), n, 1, None) == 0
    got = _host(Cd)
    print("create_dv + product: %.3f s" % (time.perf_counter() - t0))
    lib.crp_csr_dev_destroy(C.byref(h))
    bad = np.flatnonzero((got != C_exact).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:5], "first row of the second trip: %d" % P.GATHER_CAP)


def test_comm_size_past_the_grid_caps(crp, orc, gpu):
    """270 149 rows (comm_mark_kernel's second trip) naming columns either side of column 8 388 608 out of 8 458 609
    (comm_count_kernel's second trip): equal to the host planner and to the oracle, for P = 1, 3, 8 and a ragged partition."""
    from crp_spmm_amd import hip, planner
    rp, ci, va, ncol = P.comm_case()
    nrow = rp.size - 1
    assert nrow > P.GATHER_CAP and (ncol + 31) // 32 > P.COUNT_WORDS_CAP
    A = hip.CsrDev(nrow, ncol, rp, ci, va)
    t0 = time.perf_counter()
    for tag, rb, xd in P.comm_partitions(planner, rp, nrow, ncol):
        ref_sizes, ref_tot = planner.csr_mat_row_part_comm_size(ncol, rp, ci, rb, xd)
        got_sizes, got_tot = A.row_part_comm_size(rb, xd)
        assert np.array_equal(ref_sizes, got_sizes) and ref_tot == got_tot, tag
        o_sizes, o_tot = orc.csr_row_part_comm_size(ncol, rp, ci, rb, xd)
        assert np.array_equal(np.asarray(o_sizes), got_sizes) and int(o_tot) == got_tot, (tag, "oracle")
    print("comm sizes: %.3f s" % (time.perf_counter() - t0))
    A.free()
