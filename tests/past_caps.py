"""Shapes past the launch-grid caps and chunk limits of the device kernels, and their data (helper module of
tests/test_gpu_past_caps.py and tests/test_past_caps_data.py; not a conftest).

Every kernel named below caps its grid, or walks its work in chunks, and past a size threshold a code path runs that never runs
below it: the second trip of a grid-stride loop, the carry of the scan's second chunk, the second row a workgroup sorts in its
scratch slice.  Each threshold is written once here, next to the source line it mirrors; each generator gives a shape past its
threshold and says what a dropped trip would leave behind.  The matrices are sparse but large: the thresholds are reached with
row and column COUNTS, not with nonzeros, wherever the code allows it.

All generators are deterministic and build CSR with unsorted columns inside the rows."""
import functools
import math

import numpy as np

import softmax_ref as R

# ---- the thresholds ---------------------------------------------------------------------------------------------------
SCAN_TILE = 2048                      # csrc/scan_sort.h:15     SCAN_THREADS * SCAN_ITEMS = 256 * 8 entries per tile
SCAN_CHUNK_TILES = 1024               # csrc/scan_sort.h:60     k_scan_block_sums: `b0 += 1024`, one trip per 1024 tile sums
SCAN_CHUNK = SCAN_CHUNK_TILES * SCAN_TILE                  # 2 097 152 entries: the longest scan with one trip and no carry
PASS1_CAP = 65536 * 256               # csrc/transpose_kernels.hip:193 (k_check_count), :200 (k_tiers);
#                                       csrc/permute_kernels.hip:192 (k_scatter_lengths): min(.., 1 << 16) blocks of 256 threads
WAVE_ROWS_CAP = (1 << 20) * 4         # csrc/transpose_kernels.hip:216 (k_fill_keys), :222 (k_sort_short);
#                                       csrc/permute_kernels.hip:208 (k_sort_short): min(.., 1 << 20) blocks of 4 waves
LDS_PAIRS = 4096                      # csrc/scan_sort.h:12     longest row sorted in LDS; longer ones go to k_sort_long
WAVE = 64                             # csrc/scan_sort.h:11
LONG_GRID = 256                       # csrc/transpose_kernels.hip:236, csrc/permute_kernels.hip:224: min(n_long, 256, budget / ..)
LONG_BUDGET = 256 << 20               # csrc/transpose_kernels.hip:235, csrc/permute_kernels.hip:223: bytes of scratch per call
LONG_FULL_GRID_MAX = LONG_BUDGET // (LONG_GRID * 8)        # 131 072: a longer row's slice leaves the budget fewer than 256 slices
SM_GRID = 2048                        # csrc/softmax_kernels.hip:231  sm_grid: min((nrow + 3) / 4, 2048) workgroups of 256 threads
GATHER_CAP = 65536 * 4                # csrc/hip_api.hip:640 (gather_row_vals_kernel), csrc/row_kernels.hip:537 (comm_mark_kernel):
#                                       min((nrow + 3) / 4, 65536) blocks of 4 waves, one wave per row
COUNT_WORDS_CAP = 1024 * 256          # csrc/row_kernels.hip:542 (comm_count_kernel): min(.., 1024) blocks of 256 threads, one word each
COUNT_COLS_CAP = COUNT_WORDS_CAP * 32                      # 8 388 608 columns


def scan_tiles(n):
    """csrc/scan_sort.h:91"""
    return (n + SCAN_TILE - 1) // SCAN_TILE


def scan_trips(n):
    """trips of the loop of k_scan_block_sums over the tile sums of an n-entry scan"""
    return (scan_tiles(n) + SCAN_CHUNK_TILES - 1) // SCAN_CHUNK_TILES


def long_grid(n_long, max_long):
    """the grid of k_sort_long and the slice (in keys) of each of its workgroups (csrc/transpose_kernels.hip:233-236)"""
    slice_ = LDS_PAIRS
    while slice_ < max_long:
        slice_ <<= 1
    return max(1, min(n_long, LONG_GRID, LONG_BUDGET // (slice_ * 8))), slice_


def sm_rows_per_trip(lpr):
    """rows one trip of the softmax kernels' row loop covers with the capped grid: 2048 workgroups of 256 / LPR row groups"""
    return SM_GRID * (256 // lpr)


def scan_model(x, carry=True):
    """The three kernels of exclusive_scan_inplace (csrc/scan_sort.h:45-101) in numpy: tile sums, the scan of the tile sums in
    chunks of 1024 with a carry from chunk to chunk, the tiles again.  carry=False drops the carry: what a second trip that
    starts from zero again would give."""
    x = np.asarray(x, np.int64)
    nb = scan_tiles(x.size)
    pad = np.zeros(nb * SCAN_TILE, np.int64)
    pad[:x.size] = x
    tiles = pad.reshape(nb, SCAN_TILE)
    bsum = tiles.sum(axis=1)
    ex = np.zeros(nb, np.int64)
    run = 0
    for b0 in range(0, nb, SCAN_CHUNK_TILES):
        chunk = bsum[b0:b0 + SCAN_CHUNK_TILES]
        ex[b0:b0 + SCAN_CHUNK_TILES] = (run if carry else 0) + np.cumsum(chunk) - chunk
        run += int(chunk.sum())
    out = ex[:, None] + np.cumsum(tiles, axis=1) - tiles
    return out.reshape(-1)[:x.size].astype(np.int32)


# ---- CSR from coordinates ----------------------------------------------------------------------------------------------

def csr_from_coo(nrow, rows, cols, rng):
    """(rowptr, colidx, val): the entries in a random order inside every row (unsorted columns), values standard normal"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    shuffle = rng.permutation(rows.size)
    rows, cols = rows[shuffle], cols[shuffle]
    order = np.argsort(rows, kind="stable")
    rp = np.zeros(nrow + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=nrow))
    return rp.astype(np.int32), cols[order].astype(np.int32), rng.standard_normal(rows.size)


def _distinct(n, count, rng):
    """`count` distinct numbers of [0, n): an arithmetic progression modulo n with a stride coprime to n"""
    assert count <= n
    while True:
        stride = int(rng.integers(1, n))
        if math.gcd(stride, n) == 1:
            break
    return (int(rng.integers(0, n)) + stride * np.arange(count, dtype=np.int64)) % n


def coo_with_column_counts(nrow, counts, rng):
    """(rows, cols) with counts[c] entries in column c, the entries of a column in distinct rows"""
    cols = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    rows = np.concatenate([_distinct(nrow, int(c), rng) for c in counts if c > 0] or [np.zeros(0, np.int64)])
    return rows, cols


def _with_duplicates(rows, cols, k):
    """the first k pairs once more: duplicate (row, column) pairs keep their original order (the tie rule)"""
    return np.concatenate([rows, rows[:k]]), np.concatenate([cols, cols[:k]])


# ---- 1. the scan, through the transpose --------------------------------------------------------------------------------
SCAN_SMALL_N = (2047, 2048, 2049, 4096, 4097)                               # ncol + 1: the tile edges
SCAN_LARGE_NCOL = (SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 3 * SCAN_TILE + 5)   # 1024 tiles (one trip), 1025 and 1028 tiles
SCAN_NCOLS = tuple(n - 1 for n in SCAN_SMALL_N) + SCAN_LARGE_NCOL


@functools.lru_cache(maxsize=None)
def scan_case(ncol):
    """(rp, ci, va, ncol) of a 20 000-row matrix for the scan over ncol + 1 counts: random columns (every tile of 2048 counts
    holds some), plus the first and last column of the first tile, of the last tile of the first chunk of 1024 tiles and of every
    later tile, and the last column; unsorted rows, 500 duplicate pairs"""
    rng = np.random.default_rng(ncol)
    nrow = 20000
    nnz = 300000 if ncol > 100000 else 6000
    tiles = scan_tiles(ncol + 1)
    named = [0, SCAN_TILE - 1, ncol - 1]
    for t in [SCAN_CHUNK_TILES - 1] + list(range(SCAN_CHUNK_TILES, tiles)):
        if t < tiles:
            named += [t * SCAN_TILE, min((t + 1) * SCAN_TILE, ncol) - 1]
    named = np.array([c for c in named if 0 <= c < ncol], np.int64)
    cols = np.concatenate([rng.integers(0, ncol, nnz), np.repeat(named, 3)])
    rows = rng.integers(0, nrow, cols.size)
    rows, cols = _with_duplicates(rows, cols, 500)
    out = csr_from_coo(nrow, rows, cols, rng) + (ncol,)
    for a in out[:3]:
        a.setflags(write=False)
    return out


# ---- 2. the transpose past its grid caps --------------------------------------------------------------------------------
BIG_N = 4200000                      # rows and columns of the big matrix: 4 entries per row, 16 800 000 nonzeros
BIG_MID_COL, BIG_LONG_COL = WAVE_ROWS_CAP + 7, WAVE_ROWS_CAP + 1000


@functools.lru_cache(maxsize=None)
def big_square():
    """(rp, ci, va, n): n = 4 200 000 rows and columns, four entries per row -- columns i + 77, i, i + 5003, i + 1 (mod n), in that
    unsorted order -- so nnz = 16 800 000.  Every 700th row names the long column (6000 entries) instead of i + 77, every 9001st
    row the mid-tier column (467 entries) instead of i; every 1013th row repeats column i + 1 (a duplicate pair).  Rows, columns
    and nonzero positions lie on both sides of every cap."""
    n = BIG_N
    i = np.arange(n, dtype=np.int64)
    ci = np.empty((n, 4), np.int32)
    ci[:, 0] = (i + 77) % n
    ci[:, 1] = i
    ci[:, 2] = (i + 5003) % n
    ci[:, 3] = (i + 1) % n
    ci[::700, 0] = BIG_LONG_COL
    ci[::9001, 1] = BIG_MID_COL
    ci[::1013, 2] = ci[::1013, 3]
    rp = (4 * np.arange(n + 1, dtype=np.int64)).astype(np.int32)
    va = np.random.default_rng(17).random(4 * n)
    out = (rp, ci.reshape(-1), va, n)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def sort_transpose(rp, ci, va, ncol):
    """tests/test_transpose.py::numpy_transpose by ONE sort of the 64-bit numbers (column << 32 | position): ascending columns,
    ascending positions inside a column -- the stable order -- several times faster than a stable argsort at 17 M entries"""
    rp, ci = np.asarray(rp, np.int32), np.asarray(ci, np.int32)
    key = (ci.astype(np.int64) << 32) | np.arange(ci.size, dtype=np.int64)
    key.sort()
    order = (key & 0xFFFFFFFF).astype(np.int32)
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    rowptr_t = np.zeros(ncol + 1, np.int64)
    rowptr_t[1:] = np.cumsum(np.bincount(ci, minlength=ncol))
    return rowptr_t.astype(np.int32), rows[order], np.asarray(va, np.float64)[order], order


TALL_NROW, TALL_NCOL = PASS1_CAP + 1000, PASS1_CAP + 1500
TALL_MID_COL, TALL_LONG_COL = PASS1_CAP + 99, PASS1_CAP + 555


@functools.lru_cache(maxsize=None)
def tall_wide():
    """(rp, ci, va, ncol): 16 778 216 rows, 16 778 716 columns, about 10^5 nonzeros: 90 000 random (row, column) pairs, the rows
    either side of both row caps and the last row, a mid-tier column (700 entries) and a long column (5000) past column
    16 777 216, duplicates"""
    rng = np.random.default_rng(23)
    rows = rng.integers(0, TALL_NROW, 90000)
    cols = rng.integers(0, TALL_NCOL, 90000)
    edge_rows = np.array([0, WAVE_ROWS_CAP - 1, WAVE_ROWS_CAP, PASS1_CAP - 1, PASS1_CAP, PASS1_CAP + 1, TALL_NROW - 1], np.int64)
    rows = np.concatenate([rows, np.repeat(edge_rows, 3), _distinct(TALL_NROW, 700, rng), _distinct(TALL_NROW, 5000, rng)])
    cols = np.concatenate([cols, rng.integers(0, TALL_NCOL, 3 * edge_rows.size), np.full(700, TALL_MID_COL), np.full(5000, TALL_LONG_COL)])
    extra = rng.integers(PASS1_CAP, TALL_NROW, 3000)                        # a few thousand entries in the rows past the cap
    rows = np.concatenate([rows, extra])
    cols = np.concatenate([cols, rng.integers(0, TALL_NCOL, extra.size)])
    rows, cols = _with_duplicates(rows, cols, 500)
    out = csr_from_coo(TALL_NROW, rows, cols, rng) + (TALL_NCOL,)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _long_counts(which, rng):
    """column (or row) counts of the two long-queue shapes, and the number of rows (columns) the entries need.
    many:   300 lengths 4097 .. 9000 (both the 8192- and the 16 384-key paddings in one 16 384-key slice) among 700 short ones:
            n_long = 300 > 256, so 44 workgroups sort a second row in their slice
    budget: one of 140 000 (a slice of 262 144 keys, 2 MiB: the budget allows 128 workgroups) and 200 of 4097 .. 4200"""
    if which == "many":
        counts = rng.integers(0, 50, 1000)
        pos = rng.choice(1000, 300, replace=False)
        counts[pos] = np.linspace(LDS_PAIRS + 1, 9000, 300).astype(np.int64)[rng.permutation(300)]
        counts[pos[:3]] = (8191, 8192, 8193)
        return counts, 9500
    assert which == "budget"
    counts = rng.integers(0, 50, 600)
    pos = rng.choice(600, 201, replace=False)
    counts[pos[1:]] = rng.integers(LDS_PAIRS + 1, 4201, 200)
    counts[pos[0]] = 140000
    return counts, 150000


LONG_CASES = ("many", "budget")


@functools.lru_cache(maxsize=None)
def long_columns(which):
    """(rp, ci, va, ncol) whose COLUMN counts are _long_counts(which): the long-row queue of the transpose"""
    rng = np.random.default_rng(31 + LONG_CASES.index(which))
    counts, nrow = _long_counts(which, rng)
    rows, cols = coo_with_column_counts(nrow, counts, rng)
    short = np.flatnonzero(counts[cols] < 50)[:300]                         # duplicate pairs, in the short columns only
    rows, cols = np.concatenate([rows, rows[short]]), np.concatenate([cols, cols[short]])
    out = csr_from_coo(nrow, rows, cols, rng) + (len(counts),)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def long_census(lens):
    """(n_long, max_long) as pass 1 / pass 2 count them"""
    lens = np.asarray(lens)
    longs = lens[lens > LDS_PAIRS]
    return int(longs.size), int(longs.max()) if longs.size else 0


# ---- 3. the permutation past the same caps -------------------------------------------------------------------------------
PERM_N = PASS1_CAP + 3001


@functools.lru_cache(maxsize=None)
def tall_square():
    """(rp, ci, va, perm): 16 780 217 rows and columns, about 2 10^5 nonzeros: random rows of 1 .. 4 entries on both sides of
    4 194 304 and 16 777 216 (the rows at the caps themselves included), a mid-tier row (900 entries) and a long row (6000) past
    row 4 194 304, random columns with repeats, a random permutation"""
    rng = np.random.default_rng(41)
    n = PERM_N
    lens = np.zeros(n, np.int64)
    pick = np.unique(np.concatenate([rng.integers(0, n, 70000), rng.integers(PASS1_CAP, n, 1500),
                                     [0, WAVE_ROWS_CAP - 1, WAVE_ROWS_CAP, PASS1_CAP - 1, PASS1_CAP, n - 1]]))
    lens[pick] = rng.integers(1, 5, pick.size)
    lens[WAVE_ROWS_CAP + 12345] = 900
    lens[PASS1_CAP - 4321] = 6000
    lens[PASS1_CAP + 77] = 130
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, n, rp[-1]).astype(np.int32)
    out = (rp.astype(np.int32), ci, rng.standard_normal(int(rp[-1])), rng.permutation(n).astype(np.int32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def long_rows(which):
    """(rp, ci, va, perm) of a square matrix whose ROW lengths are _long_counts(which): the long-row queue of the permutation;
    columns random with repeats"""
    rng = np.random.default_rng(51 + LONG_CASES.index(which))
    lens, n = _long_counts(which, rng)
    lens = np.concatenate([lens, rng.integers(0, 3, n - lens.size)])[rng.permutation(n)]
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    out = (rp.astype(np.int32), rng.integers(0, n, rp[-1]).astype(np.int32), rng.standard_normal(int(rp[-1])),
           rng.permutation(n).astype(np.int32))
    for a in out:
        a.setflags(write=False)
    return out


# ---- 4. the row softmax past sm_grid --------------------------------------------------------------------------------------
SM_LPRS = (8, 16, 32, 64)
_SM_BASE = {8: (0, 11), 16: (4, 25), 32: (10, 45), 64: (30, 91)}            # base row lengths [lo, hi): means 5, 14, 27, 60
SM_WINDOW = 300                                                              # rows of the small calls on a later trip


def sm_nrow(lpr):
    """more than three trips, the last one partial and ending inside a workgroup (not a multiple of the 256 / LPR row groups)"""
    n = 3 * sm_rows_per_trip(lpr) + 1000 + 3
    assert n % (256 // lpr) != 0
    return n


def sm_windows(lpr):
    """(r0, r1) of the second and of the third trip: the special rows of those trips lie inside"""
    t = sm_rows_per_trip(lpr)
    return (t + 5, t + 5 + SM_WINDOW), (2 * t + 7, 2 * t + 7 + SM_WINDOW)


def sm_special_rows(lpr):
    """{row: (length, all masked)} inside the windows of the second and third trip: an empty row, a masked register row, a
    masked row over memory, a register row at its limit of 8 LPR entries, one entry more, a long row, rows of one and two"""
    out = {}
    for r0, _r1 in sm_windows(lpr):
        for k, spec in enumerate(((0, False), (5, True), (8 * lpr + 9, True), (8 * lpr, False), (8 * lpr + 1, False),
                                  (20 * lpr + 3, False), (1, False), (2, False), (0, False), (8 * lpr + 70, False))):
            out[r0 + 10 + 7 * k] = spec
    return out


@functools.lru_cache(maxsize=None)
def sm_rowptr(lpr):
    rng = np.random.default_rng(60 + lpr)
    n = sm_nrow(lpr)
    lens = rng.integers(*_SM_BASE[lpr], n)
    lens[rng.random(n) < 0.04] = 0                                           # empty rows everywhere
    over = rng.choice(n, 120, replace=False)                                 # rows over memory in every trip
    lens[over] = rng.integers(8 * lpr + 1, 12 * lpr, over.size)
    for r, (length, _masked) in sm_special_rows(lpr).items():
        lens[r] = length
    lens[n - 1] = 8 * lpr + 2                                                # the last row of the partial trip
    rp = R.rowptr_of(lens)
    rp.setflags(write=False)
    return rp


@functools.lru_cache(maxsize=None)
def sm_case(lpr, dtype):
    """(rp, s, ref, bound, y, dy, ref_bwd, bound_bwd) as softmax_ref.case gives them, on sm_rowptr(lpr): spread 8, one masked
    entry per row, the masked special rows entirely -inf; y is the replay's forward result -- the y the backward reads"""
    dt = np.dtype(dtype)
    rp = sm_rowptr(lpr)
    seed = 7000 + 2 * lpr + (dt == np.float32)
    s = R.scores(rp, dt, 8, seed)
    for r, (_length, masked) in sm_special_rows(lpr).items():
        if masked:
            s[rp[r]:rp[r + 1]] = -np.inf
    ref, L, T = R.reference_fwd(rp, s)
    y = R.replay_fwd(rp, s)
    dy = R.grads(s.size, dt, seed + 100000)
    rb, Lb, S = R.reference_bwd(rp, y, dy)
    out = (rp, s, ref, R.bound_fwd(ref, L, T, dt), y, dy, rb, R.bound_bwd(y, dy, Lb, S, dt))
    for a in out:
        a.setflags(write=False)
    return out


# ---- 5. the gather of crp_csr_dev_create_dv and the planner's comm-size kernels ------------------------------------------
GATHER_FULL_ROWS, GATHER_SUB_ROWS, GATHER_NCOL = 300000, GATHER_CAP + 7003, 4096


@functools.lru_cache(maxsize=None)
def gather_case():
    """(full_rp, rows, sub_rp, sub_ci, start): a 300 000-row pattern of about 3 entries per row with rows of 65 .. 200 entries
    mixed in, and the subset of 269 147 of its rows (ascending) that the handle is made of; start[t] = full_rp[rows[t]]"""
    rng = np.random.default_rng(71)
    lens = rng.integers(0, 7, GATHER_FULL_ROWS)
    fat = rng.choice(GATHER_FULL_ROWS, 400, replace=False)
    lens[fat] = rng.integers(65, 201, fat.size)
    full_rp = R.rowptr_of(lens)
    rows = np.sort(rng.choice(GATHER_FULL_ROWS, GATHER_SUB_ROWS, replace=False)).astype(np.int32)
    rows = np.union1d(rows, fat[:200])[:GATHER_SUB_ROWS].astype(np.int32)
    sub_rp = R.rowptr_of(lens[rows])
    sub_ci = rng.integers(0, GATHER_NCOL, int(sub_rp[-1])).astype(np.int32)
    start = np.ascontiguousarray(full_rp[rows], dtype=np.int32)
    out = (full_rp, rows, sub_rp, sub_ci, start)
    for a in out:
        a.setflags(write=False)
    return out


def gather_index(full_rp, rows, sub_rp):
    """position in the full matrix's values of every entry of the subset: sub_val = full_val[gather_index]"""
    lens = np.diff(sub_rp)
    return np.repeat(full_rp[rows].astype(np.int64) - sub_rp[:-1], lens) + np.arange(int(sub_rp[-1]), dtype=np.int64)


COMM_NROW, COMM_NCOL = GATHER_CAP + 8005, COUNT_COLS_CAP + 70001


@functools.lru_cache(maxsize=None)
def comm_case():
    """(rp, ci, va, ncol): 270 149 rows of 0 .. 6 random columns out of 8 458 609, with a cluster of named columns either side of
    column 8 388 608 (word 262 144 of a block's bitmap) and the last column"""
    rng = np.random.default_rng(81)
    lens = rng.integers(0, 7, COMM_NROW)
    rows = np.repeat(np.arange(COMM_NROW, dtype=np.int64), lens)
    cols = rng.integers(0, COMM_NCOL, rows.size)
    near = np.concatenate([np.arange(COUNT_COLS_CAP - 40, COUNT_COLS_CAP + 40), [COMM_NCOL - 1, 0]])
    rows = np.concatenate([rows, rng.integers(0, COMM_NROW, near.size), rng.integers(GATHER_CAP, COMM_NROW, near.size)])
    cols = np.concatenate([cols, near, near])
    out = csr_from_coo(COMM_NROW, rows, cols, rng) + (COMM_NCOL,)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def comm_partitions(planner, rp, nrow, ncol):
    """(tag, rblk, xd): the planner's nnz-balanced row blocks for P = 1, 3, 8 with an even column partition, and a ragged pair
    (empty blocks at both ends, a column partition unrelated to the rows, one edge inside word 262 144)"""
    for P in (1, 3, 8):
        yield "P=%d" % P, planner.csr_mat_row_partition(rp, P), planner.even_displs(ncol, P)
    rb = np.array([0, 0, nrow // 3, nrow // 3, GATHER_CAP + 1, nrow, nrow], dtype=np.int32)
    xd = np.array([0, ncol // 5, ncol // 5, ncol // 2, COUNT_COLS_CAP + 13, ncol - 1, ncol], dtype=np.int32)
    yield "ragged", rb, xd
