"""Operands past 2^31 elements (fp32) and past 2^32 bytes (fp64) for the pattern and row kernels: the arena, its layout, the
patterns and the case table (helper module of tests/test_gpu_far_rows.py and tests/test_far_rows_data.py; not a conftest;
DESIGN.md 5u).

Every device kernel since the SpMM kernels forms a row address as base + (int64_t) index * ld.  A case here places every 2-D
operand of one call as a strided view into ONE arena with ld = 2^20 (the 16-byte instances) or 2^20 + 1 (the element instances),
so that the last 64 rows of every operand -- the FAR rows -- lie at offsets no 32-bit number holds, and compares the call with
the same call on compact copies.  The arena is laid out so that an address truncated to 32 bits, in any of the four ways below,
stays inside the allocation and lands on other data: a narrowed offset shows as wrong bits, never as a stray access.

    tier      arena rows   operand base   operand rows   far rows       what is past 32 bits there
    float32   4160         row 2048       2112           2048 .. 2111   the element offset (>= 2^31) and the byte offset (>= 2^33)
    float64    832         row  256        576            512 ..  575   the byte offset (>= 2^32); elements stay below 2^31

Wrap models (of the offset the kernel adds to an operand's pointer): the element offset as int32 / uint32, the byte offset as
int32 / uint32.  REACHED says which of them move a far address in which tier; the unsigned element wrap needs offsets of 2^32
elements (16 GiB more in fp32, 32 GiB in fp64) and is reached in neither.

Nothing here needs a device or the library."""
import collections
import functools

import numpy as np

SENT = -77.0                             # the project's finite sentinel: the arena's fill
LD_VEC, LD_ELEM = 1 << 20, (1 << 20) + 1
LD = {"vec": LD_VEC, "elem": LD_ELEM}    # instance -> leading dimension
INSTANCES = ("vec", "elem")
DTYPES = ("float32", "float64")
W = 4096                                 # operands live in columns [0, W) of their rows
FAR = 64                                 # far rows per operand, decoy rows per arena
DECOY_W = 2 * W                          # decoy rows hold data in columns [0, DECOY_W): with ld = 2^20 + 1 a wrapped address
#                                          of column c lands on column 4096 + c of its decoy row
WIDTHS = {"vec": (8, 40), "elem": (7, 33)}            # one head's width
DROP, SEED = 0.5, 0x1234567800000001     # the dropout cases (tests/dropout_ref.py's rate and seed)

Tier = collections.namedtuple("Tier", "dtype itemsize rows base m far0")
TIERS = {"float32": Tier("float32", 4, 4160, 2048, 2112, 2048), "float64": Tier("float64", 8, 832, 256, 576, 512)}


def arena_elems(dtype):
    """elements of the arena: `rows` rows of 2^20 + 1 (the slack of the odd ld: one element per row)"""
    return TIERS[dtype].rows * LD_ELEM


def arena_bytes(dtype):
    return arena_elems(dtype) * TIERS[dtype].itemsize


# ---- operands and where they go -------------------------------------------------------------------------------------------

Op = collections.namedtuple("Op", "name rows width out")                 # a 2-D operand of a call: `out` = the call writes it
Placed = collections.namedtuple("Placed", "name rows width out row0 col ld")


def vw(dtype):
    return 16 // TIERS[dtype].itemsize


def place(dtype, inst, ops):
    """name -> Placed: the operands side by side in columns [0, W) from the tier's base row; column offsets are multiples of 4
    elements (vec) or odd (elem)"""
    tier, ld = TIERS[dtype], LD[inst]
    out, col = {}, 0
    for op in ops:
        col = (col + 3) // 4 * 4 if inst == "vec" else col | 1
        assert col + op.width <= W and op.rows <= tier.m, (op, col)
        out[op.name] = Placed(op.name, op.rows, op.width, op.out, tier.base, col, ld)
        col += op.width
    return out


def compact_layout(dtype, inst, width):
    """(ld, storage offset) of the compact copy of an operand of `width` columns: a multiple of the vector width on a 16-byte
    pointer (vec); odd, one element into its allocation (elem)"""
    if inst == "vec":
        v = vw(dtype)
        return (width + v - 1) // v * v, 0
    return width | 1, 1


def alignment_class(dtype, elem_offset, ld):
    """what the kernels' instance choice looks at: the pointer modulo 16 and 8 bytes and the leading dimension modulo the
    vector width and 2 (the pointer as its element offset from a 16-byte aligned allocation)"""
    size = TIERS[dtype].itemsize
    return ((elem_offset * size) % 16 == 0, (elem_offset * size) % 8 == 0, ld % vw(dtype) == 0, ld % 2 == 0)


# ---- the wrap models ------------------------------------------------------------------------------------------------------

WRAPS = ("elem_i32", "elem_u32", "byte_i32", "byte_u32")
REACHED = {("float32", "elem_i32"): True, ("float32", "elem_u32"): False, ("float32", "byte_i32"): True, ("float32", "byte_u32"): True,
           ("float64", "elem_i32"): False, ("float64", "elem_u32"): False, ("float64", "byte_i32"): True, ("float64", "byte_u32"): True}


def wrap(off, model, itemsize):
    """the element offset(s) `off` (int64, >= 0) as a kernel would form them with the offset narrowed by `model`"""
    off = np.asarray(off, np.int64)
    unit = itemsize if model.startswith("byte") else 1
    x = (off * unit) & 0xFFFFFFFF
    if model.endswith("i32"):
        x = np.where(x >= 1 << 31, x - (1 << 32), x)
    assert (x % unit == 0).all()
    return x // unit


def offsets(p):
    """element offsets from the operand's pointer of its first and last column in every row: (rows, 2)"""
    return np.arange(p.rows, dtype=np.int64)[:, None] * p.ld + np.array([0, p.width - 1], np.int64)[None, :]


def base_offset(p):
    """element offset of the operand's pointer from the arena's"""
    return p.row0 * p.ld + p.col


def content(dtype, ld, pos):
    """what lies at the arena elements `pos` under leading dimension ld: (kind, arena row) with kind 2 = columns [0, W) of the
    operand rows, 1 = a decoy row's data, 0 = sentinel"""
    tier = TIERS[dtype]
    row, col = pos // ld, pos % ld
    kind = np.where((row >= tier.base) & (row < tier.base + tier.m) & (col < W), 2, np.where((row < FAR) & (col < DECOY_W), 1, 0))
    return kind, row


# ---- the patterns -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pattern(dtype):
    """dict(m, rp, ci, val, codes, empty) of the tier's matrix, m = k = the operand row count: rows of 12 .. 20 entries in a random
    order (unsorted, distinct columns), each with a far and a near column at least; every 97th near row is empty, no far row is;
    every far column is named.  codes: the two-source form -- about a third of the entries, one of every row's far ones among
    them, read row c of the second source instead (code ~c).  val: standard normal."""
    tier = TIERS[dtype]
    m, far0 = tier.m, tier.far0
    rng = np.random.default_rng(100 + tier.itemsize)
    lens = rng.integers(12, 21, m)
    empty = np.arange(5, far0, 97)
    lens[empty] = 0
    cols, codes = [], []
    for i in range(m):
        if lens[i] == 0:
            continue
        far = rng.choice(np.arange(far0, m), size=2, replace=False)
        far[0] = far0 + (i % FAR)                                          # (every far column is named, whatever the draw)
        if far[1] == far[0]:
            far[1] = far0 + (i + 1) % FAR
        near = rng.choice(far0, size=lens[i] - 2, replace=False)
        row = np.concatenate([far, near])
        second = rng.random(row.size) < 0.3
        second[0], second[1] = True, False                                 # a far row of either source
        order = rng.permutation(row.size)
        cols.append(row[order])
        codes.append(np.where(second, ~row, row)[order])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    out = dict(m=m, rp=rp, ci=np.concatenate(cols).astype(np.int32), codes=np.concatenate(codes).astype(np.int32),
               val=rng.standard_normal(int(rp[-1])), empty=empty)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def rows_of(rp):
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def row_data(rng, rows, width, dtype, integers=False):
    """an operand's data: standard normal in the dtype, or small integers (sums of up to 2112 of them are exact in fp32)"""
    if integers:
        return rng.integers(-8, 9, (rows, width)).astype(dtype)
    return rng.standard_normal((rows, width)).astype(dtype)


def dot_reference(rp, ci, X, Y, chunk=2048):
    """(ref, S) per nonzero in np.longdouble: ref = <X[i], Y[c]>, S = sum_j |x_j y_j| -- what the SDDMM's bound (n + 1) u S of
    DESIGN.md 5d takes (mode 0; any order of an n-term dot errs by at most gamma_n S)"""
    rows = rows_of(rp)
    Xl, Yl = X.astype(np.longdouble), Y.astype(np.longdouble)
    ref, S = np.empty(ci.size, np.longdouble), np.empty(ci.size, np.longdouble)
    for a in range(0, ci.size, chunk):
        prod = Xl[rows[a:a + chunk]] * Yl[ci[a:a + chunk]]
        ref[a:a + chunk], S[a:a + chunk] = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    return ref, S


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (0 / 0 = 0, x / 0 = inf); a non-finite entry of got counts as inf"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got.astype(np.longdouble) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def decoy_data(dtype):
    """(FAR, DECOY_W) in [100, 200): no operand holds such a value"""
    return (100 + 100 * np.random.default_rng(9).random((FAR, DECOY_W))).astype(dtype)


def move_lists(m, seed=4):
    """(perm, seg_row, seg_ptr, seg_pos) of the row moves: a permutation of the m rows with far rows moved to near ones and near
    to far; for scatter_add_rows, 300 distinct destination rows -- the far ones among them -- of 0 .. 5 source rows each, far
    sources in every far destination's list"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(m).astype(np.int32)
    near = rng.choice(m - FAR, size=300 - FAR, replace=False)
    seg_row = rng.permutation(np.concatenate([near, np.arange(m - FAR, m)])).astype(np.int32)
    lens = rng.integers(0, 6, seg_row.size)
    lens[seg_row >= m - FAR] = np.maximum(lens[seg_row >= m - FAR], 2)
    seg_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    seg_pos = rng.integers(0, m, int(seg_ptr[-1])).astype(np.int32)
    first = seg_ptr[:-1][seg_row >= m - FAR]
    seg_pos[first] = rng.integers(m - FAR, m, first.size)
    return perm, seg_row, seg_ptr, seg_pos


# ---- the per-edge index times heads -------------------------------------------------------------------------------------------

POS_HEADS = 8
POS_ROWS = (1 << 28) + FAR               # rows of the (POS_ROWS, 8) output view; entries of row >= 2^28 lie at index >= 2^31
POS_BASE = 1 << 31                       # the view starts this many elements (the mask: bytes) into the arena
POS_CALLS = ("attention.p_out", "gat_attention.p_out", "gat_attention_bwd_row.ds_out", "dropout_mask")


def out_positions(nnz, seed=6):
    """out_pos of nnz distinct rows of the view: 2^28 .. 2^28 + 63 and nnz - 64 rows below 2^28, in a random order"""
    rng = np.random.default_rng(seed)
    low = np.unique(rng.integers(0, 1 << 28, 2 * nnz))[:nnz - FAR]
    assert low.size == nnz - FAR
    return rng.permutation(np.concatenate([low, (1 << 28) + np.arange(FAR)])).astype(np.int32)


# ---- the case table ---------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "id family call kw")


def _cases():
    out = [Case("sddmm-1src", "sddmm", "sddmm", dict(sources=1)), Case("sddmm-2src", "sddmm", "sddmm", dict(sources=2))]
    for H in (1, 2):
        for call in ("attention", "attention_bwd_q", "attention_bwd_kv"):
            out.append(Case("%s-h%d" % (call, H), "attention", call, dict(heads=H)))
    for fam in ("gat", "gatv2"):
        for drop in (0.0, DROP):
            for side in ("", "_bwd_row", "_bwd_col"):
                call = "%s_attention%s" % (fam, side)
                out.append(Case(call + ("-drop" if drop else ""), fam, call, dict(heads=2, dropout=drop)))
    for call in ("gather_rows", "scatter_rows"):
        for layout in (0, 1):
            out.append(Case("%s-layout%d" % (call, layout), "rows", call, dict(layout=layout)))
    out += [Case("transpose-src-far", "rows", "transpose", dict(far="src")), Case("transpose-dst-far", "rows", "transpose", dict(far="dst")),
            Case("scatter_add_rows", "rows", "scatter_add_rows", {}), Case("sum_segments", "rows", "sum_segments", {}),
            Case("col_sum", "rows", "col_sum", {})]
    return tuple(out)


CASES = _cases()
CASE_BY_ID = {c.id: c for c in CASES}


def operands(case, dtype, w):
    """the 2-D operands of the case's call at one head's width w, in the order they are placed.  Vectors without a leading
    dimension (lse, delta, the per-edge outputs, GATv2's a, index lists, the results of the two sums) are contiguous by the
    calls' contracts and live outside the arena."""
    m = TIERS[dtype].m
    H = case.kw.get("heads", 1)
    full = lambda *names, out=False: [Op(n, m, H * w, out) for n in names]
    head = lambda *names, out=False: [Op(n, m, H, out) for n in names]
    c = case.call
    if c == "sddmm":
        return full("X", "Y0") + (full("Y1") if case.kw["sources"] == 2 else [])
    if c == "attention":
        return full("Q", "K", "V") + full("O", out=True)
    if c == "attention_bwd_q":
        return full("Q", "K", "V", "O", "dO") + full("dQ", out=True)
    if c == "attention_bwd_kv":
        return full("K", "V", "Q", "dO") + full("dK", "dV", out=True)
    if c == "gat_attention":
        return head("el", "er") + full("V") + full("O", out=True)
    if c == "gat_attention_bwd_row":
        return head("el", "er") + full("V", "O", "dO") + head("d_el", out=True)
    if c == "gat_attention_bwd_col":
        return head("er", "el") + full("V", "dO") + head("d_er", out=True) + full("dV", out=True)
    if c == "gatv2_attention":
        return full("XT", "XS") + full("O", out=True)
    if c == "gatv2_attention_bwd_row":
        return full("XT", "XS", "O", "dO") + full("dXT", "da_part", out=True)
    if c == "gatv2_attention_bwd_col":
        return full("XS", "XT", "dO") + full("dXS", out=True)
    if c in ("gather_rows", "scatter_rows", "scatter_add_rows"):        # (layout 1: the arena rows are the columns)
        return [Op("src", m, w, False), Op("dst", m, w, True)]
    if c == "transpose":
        a, b = Op("src", m, w, False), Op("dst", w, m, True)
        return [a, b] if case.kw["far"] == "src" else [Op("src", w, m, False), Op("dst", m, w, True)]
    if c in ("sum_segments", "col_sum"):
        return [Op("src", m, w, False)]
    raise KeyError(c)
