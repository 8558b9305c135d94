"""CPU: the layout of tests/far_rows.py, from that module alone -- the far rows are past 32 bits, every address of every case is
inside the arena, and an address narrowed to 32 bits stays inside and lands on other data (the numpy stand-in for "the GPU test
would fail, and not fault, if a kernel truncated")."""
import numpy as np
import pytest

import far_rows as FR

LAYOUTS = [(dt, inst) for dt in FR.DTYPES for inst in FR.INSTANCES]


def _placed(dtype, inst):
    """every placed operand of every case at both widths"""
    for case in FR.CASES:
        for w in FR.WIDTHS[inst]:
            for p in FR.place(dtype, inst, FR.operands(case, dtype, w)).values():
                yield case, w, p


def test_the_arena_sizes_are_the_documented_ones():
    assert FR.arena_bytes("float32") == 4160 * ((1 << 20) + 1) * 4 and abs(FR.arena_bytes("float32") / 2 ** 30 - 16.25) < 1e-4
    assert FR.arena_bytes("float64") == 832 * ((1 << 20) + 1) * 8 and abs(FR.arena_bytes("float64") / 2 ** 30 - 6.5) < 1e-4
    for dt, tier in FR.TIERS.items():
        assert tier.base + tier.m == tier.rows and tier.m - tier.far0 == FR.FAR
        assert tier.base * FR.LD_VEC * tier.itemsize in (1 << 31, 1 << 33)      # fp64: based 2^31 bytes in; fp32: 2^31 elements in
    assert FR.TIERS["float32"].base * FR.LD_VEC == 1 << 31


@pytest.mark.parametrize("dtype,inst", LAYOUTS)
def test_far_rows_are_past_32_bits(dtype, inst):
    tier, ld = FR.TIERS[dtype], FR.LD[inst]
    far = np.arange(tier.far0, tier.m, dtype=np.int64) * ld
    assert (far * tier.itemsize >= 1 << 32).all()
    if dtype == "float32":
        assert (far >= 1 << 31).all() and (far + FR.W < 1 << 32).all()
    else:
        assert (np.arange(tier.m, dtype=np.int64) * ld + FR.W < 1 << 31).all()      # fp64 pins bytes: elements stay below 2^31


@pytest.mark.parametrize("dtype,inst", LAYOUTS)
def test_every_address_of_every_case_is_inside_the_arena(dtype, inst):
    n = FR.arena_elems(dtype)
    seen = 0
    for case, w, p in _placed(dtype, inst):
        pos = FR.base_offset(p) + FR.offsets(p)
        assert pos.min() >= 0 and pos.max() < n, (case.id, w, p)
        kind, _ = FR.content(dtype, p.ld, pos)
        assert (kind == 2).all(), (case.id, w, p, "an operand leaves columns [0, W) of the operand rows")
        seen += 1
    assert seen >= 2 * len(FR.CASES)
    # operands of one call do not overlap
    for case in FR.CASES:
        for w in FR.WIDTHS[inst]:
            spans = sorted((p.col, p.col + p.width) for p in FR.place(dtype, inst, FR.operands(case, dtype, w)).values())
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (case.id, w, spans)


@pytest.mark.parametrize("model", FR.WRAPS)
@pytest.mark.parametrize("dtype,inst", LAYOUTS)
def test_a_wrapped_address_stays_inside_and_lands_on_other_data(dtype, inst, model):
    tier = FR.TIERS[dtype]
    n = FR.arena_elems(dtype)
    reached = FR.REACHED[(dtype, model)]
    for case, w, p in _placed(dtype, inst):
        off = FR.offsets(p)
        wrapped = FR.wrap(off, model, tier.itemsize)
        pos, true = FR.base_offset(p) + wrapped, FR.base_offset(p) + off
        assert pos.min() >= 0 and pos.max() < n, (case.id, w, p, model, "a wrapped address leaves the arena")
        if p.rows <= tier.far0:                                            # (the short side of a transpose has no far rows)
            assert np.array_equal(pos, true)
            continue
        far = slice(tier.far0, p.rows)
        if not reached:                                                    # the model does not move a far address in this tier
            assert np.array_equal(pos[far], true[far]), (case.id, model)
            continue
        kind, row = FR.content(dtype, p.ld, pos[far])
        _, true_row = FR.content(dtype, p.ld, true[far])
        assert (row != true_row).all(), (case.id, w, p, model, "a wrapped far address lands on its own row")
        # ... and on other data.  ld = 2^20: the same columns of another row -- the operand's own data there (no two rows are equal)
        # or a decoy row's.  ld = 2^20 + 1: a wrap by a multiple of 2^20 elements also shifts the column, so a byte wrap may land on
        # another operand's columns, on the sentinel fill of columns [0, W) or past column W: a read of -77 (no operand holds it) is
        # wrong bits too, and a write there fails the clone comparison or the sentinel reduction.
        if inst == "vec":
            assert (kind >= 1).all(), (case.id, w, p, model)
            cols = pos[far] % p.ld
            assert np.array_equal(cols, true[far] % p.ld) and ((kind == 1) | ((row >= p.row0) & (row < p.row0 + p.rows))).all()
        if dtype == "float32" and model == "elem_i32":
            assert (row < FR.FAR).all() and (kind == 1).all(), "the signed element wrap lands on the decoy rows' data"


def test_the_unsigned_element_wrap_is_the_one_not_reached():
    assert [k for k, v in FR.REACHED.items() if not v] == [("float32", "elem_u32"), ("float64", "elem_i32"), ("float64", "elem_u32")]
    assert FR.arena_elems("float32") + FR.W < (1 << 32) + (FR.FAR + 1) * FR.LD_ELEM       # no offset of 2^32 elements from an operand


@pytest.mark.parametrize("dtype", FR.DTYPES)
def test_every_pattern_names_far_rows_on_every_side(dtype):
    tier = FR.TIERS[dtype]
    pat = FR.pattern(dtype)
    m, rp, ci, codes = pat["m"], pat["rp"], pat["ci"], pat["codes"]
    assert m == tier.m and rp.size == m + 1 and rp[-1] == ci.size == codes.size == pat["val"].size
    lens = np.diff(rp)
    assert 15 <= lens[lens > 0].mean() <= 17 and (lens[tier.far0:] > 0).all() and 3 <= (lens == 0).sum() and (lens[pat["empty"]] == 0).all()
    assert ci.min() >= 0 and ci.max() < m
    unsorted = 0
    for i in np.flatnonzero(lens):
        row = ci[rp[i]:rp[i + 1]]
        assert np.unique(row).size == row.size
        assert (row >= tier.far0).any() and (row < tier.far0).any(), (i, "a far and a near column in every row")
        unsorted += bool((np.diff(row) < 0).any())
        c2 = codes[rp[i]:rp[i + 1]]
        assert (c2[c2 >= 0] >= tier.far0).any() and (~c2[c2 < 0] >= tier.far0).any(), (i, "a far row of either source")
    assert unsorted > 0.9 * np.count_nonzero(lens)
    assert (np.bincount(ci, minlength=m)[tier.far0:] > 0).all(), "the column side: every far row of the transposed handle has entries"
    assert np.array_equal(np.where(codes < 0, ~codes, codes), ci) and 0.2 < (codes < 0).mean() < 0.45
    perm, seg_row, seg_ptr, seg_pos = FR.move_lists(m)
    assert np.array_equal(np.sort(perm), np.arange(m)) and (perm[tier.far0:] < tier.far0).any() and (perm[:tier.far0] >= tier.far0).any()
    assert np.unique(seg_row).size == seg_row.size and set(range(tier.far0, m)) <= set(seg_row.tolist())
    assert (np.diff(seg_ptr) == 0).any() and seg_pos.max() < m
    for t in np.flatnonzero(seg_row >= tier.far0):
        assert (seg_pos[seg_ptr[t]:seg_ptr[t + 1]] >= tier.far0).any()
    rows = FR.row_data(np.random.default_rng(0), m, 7, dtype, integers=True)
    assert np.unique(rows, axis=0).shape[0] == m or np.unique(rows, axis=0).shape[0] > m - 3


@pytest.mark.parametrize("dtype,inst", LAYOUTS)
def test_far_views_and_compact_copies_share_an_alignment_class(dtype, inst):
    for case, w, p in _placed(dtype, inst):
        ld, off = FR.compact_layout(dtype, inst, p.width)
        assert ld >= p.width
        far_class = FR.alignment_class(dtype, FR.base_offset(p), p.ld)
        assert far_class == FR.alignment_class(dtype, off, ld), (case.id, w, p)
        eight = dtype == "float64"                                         # (every pointer to doubles is 8-byte aligned)
        assert far_class == ((True, True, True, True) if inst == "vec" else (False, eight, False, False)), (case.id, w, p)


def test_out_positions_reach_2_31_and_stay_inside():
    nnz = int(FR.pattern("float32")["rp"][-1])
    pos = FR.out_positions(nnz).astype(np.int64)
    assert pos.size == nnz and np.unique(pos).size == nnz and pos.min() >= 0 and pos.max() == (1 << 28) + FR.FAR - 1 < FR.POS_ROWS
    idx = pos * FR.POS_HEADS + (FR.POS_HEADS - 1)
    assert (idx[pos >= 1 << 28] >= 1 << 31).all() and (pos >= 1 << 28).sum() == FR.FAR and idx.max() < FR.POS_ROWS * FR.POS_HEADS
    # the view ends inside the arena, in elements (fp32 outputs) and in bytes (the mask) ...
    assert FR.POS_BASE + FR.POS_ROWS * FR.POS_HEADS <= FR.arena_elems("float32")
    # ... and an index narrowed to int32 lands on the first decoy row's data
    wrapped = FR.POS_BASE + FR.wrap(idx[pos >= 1 << 28], "elem_i32", 1)
    assert wrapped.min() >= 0 and wrapped.max() < FR.DECOY_W
