"""GPU: the streaming kernels of csrc/row_kernels.hip at the edges no other direct test reaches, bit for bit against numpy and
torch indexing, NaN payloads included.  Every destination lies inside a larger buffer whose guard columns and guard rows hold a
sentinel, and the WHOLE buffer is compared.

  * crp_gather_rows_f64 / crp_scatter_rows_f64 / crp_transpose_f64 on the grid of test_gpu_engine_f32.py's fp32 test: odd widths,
    padded leading dimensions, pointers 8 and 16 bytes off a 16-byte boundary, both layouts (scatter in layout 1, transpose with
    lds != ncol and ldd != nrow)
  * crp_scatter_add_rows_f64 / _f32: the 16-byte instance and the element instance on the same data give the same bits
  * one call per kernel with more work items than the grid cap (2048 blocks x 256 threads = 524 288), so that the second trip of
    every grid-stride loop runs under a bitwise check"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID_CAP = 2048 * 256
SENT = -7.0


def _mantissa_full(rng, shape, dt):
    """values with full mantissas over scales 2^-20 .. 2^20: the order of the additions shows in the last bits"""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, size=shape))).astype(dt)


def _payload(rng, shape, dt):
    """Full-mantissa values with NaNs of distinct payloads mixed in: a copy through any arithmetic would quiet or lose them."""
    x = _mantissa_full(rng, shape, dt)
    flat = x.reshape(-1).view(np.int64 if dt == np.float64 else np.int32)
    hit = rng.random(flat.size) < 0.03
    base, mask = (0x7FF0000000000000, (1 << 52) - 1) if dt == np.float64 else (0x7F800000, (1 << 23) - 1)
    flat[hit] = base | (1 + rng.integers(0, mask, size=int(hit.sum())))          # (signalling and quiet payloads alike)
    assert np.isnan(x).sum() == hit.sum()
    return x


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _guarded(torch, gpu, rows, cols, off, pad, dtype, data=None):
    """(full, view): a (rows + 2) x (off + cols + pad) buffer of SENT and its rows x cols interior, one guard row above and below."""
    full = torch.full((rows + 2, off + cols + pad), SENT, dtype=dtype, device=gpu)
    view = full[1:rows + 1, off:off + cols]
    if data is not None:
        view.copy_(data)
    return full, view


def _same(torch, got_full, want_full, tag):
    assert torch.equal(_bits(got_full), _bits(want_full)), tag


@pytest.mark.parametrize("n", [1, 7, 30, 64, 257])
def test_row_kernels_f64_bit_exact(crp, gpu, n):
    import torch
    from crp_spmm_amd import hip
    rng = np.random.default_rng(n)
    nsrc, nidx = 301, 173
    perm = torch.from_numpy(rng.permutation(nsrc)[:nidx].astype(np.int32)).to(gpu)           # distinct rows: a scatter has one answer
    rep = torch.from_numpy(rng.integers(0, nsrc, size=nidx).astype(np.int32)).to(gpu)        # a gather may repeat rows
    rep[5] = rep[6]
    f64 = torch.float64
    vec_calls = 0
    for off in (0, 1, 2):
        for pad in (0, 3, 8):
            tag = (n, off, pad)
            src = torch.from_numpy(_payload(rng, (nsrc, n), np.float64)).to(gpu)
            # ---- row-major
            src_full, src_v = _guarded(torch, gpu, nsrc, n, off, pad, f64, src)
            for ridx in (perm, rep):
                dst_full, dst_v = _guarded(torch, gpu, nidx, n, off, pad, f64)
                vec_calls += int(n % 2 == 0 and src_v.stride(0) % 2 == 0 and (src_v.data_ptr() | dst_v.data_ptr()) % 16 == 0)
                hip.gather_rows(ridx, src_v, dst_v)
                want_full, want_v = _guarded(torch, gpu, nidx, n, off, pad, f64)
                want_v.copy_(src[ridx.long()])
                _same(torch, dst_full, want_full, tag + ("gather",))
            out_full, out_v = _guarded(torch, gpu, nsrc, n, off, pad, f64)
            packed = src[:nidx].contiguous()
            hip.gather_rows(perm, packed, out_v, scatter=True)
            want_full, want_v = _guarded(torch, gpu, nsrc, n, off, pad, f64)
            want_v[perm.long()] = packed
            _same(torch, out_full, want_full, tag + ("scatter",))
            # ---- column-major: (n, ld) tensors, the rows of the matrix along the fast dimension
            csrc_full, csrc_v = _guarded(torch, gpu, n, nsrc, off, pad, f64, src.t())
            cdst_full, cdst_v = _guarded(torch, gpu, n, nidx, off, pad, f64)
            hip.gather_rows(rep, csrc_v, cdst_v, layout=1)
            want_full, want_v = _guarded(torch, gpu, n, nidx, off, pad, f64)
            want_v.copy_(src.t()[:, rep.long()])
            _same(torch, cdst_full, want_full, tag + ("gather, layout 1",))
            cout_full, cout_v = _guarded(torch, gpu, n, nsrc, off, pad, f64)
            cpacked_full, cpacked_v = _guarded(torch, gpu, n, nidx, off, pad, f64, src[:nidx].t())
            hip.gather_rows(perm, cpacked_v, cout_v, layout=1, scatter=True)
            want_full, want_v = _guarded(torch, gpu, n, nsrc, off, pad, f64)
            want_v[:, perm.long()] = src[:nidx].t()
            _same(torch, cout_full, want_full, tag + ("scatter, layout 1",))
            # ---- transpose: nsrc x n (lds = off + n + pad) -> n x nsrc (ldd = off + nsrc + pad)
            tdst_full, tdst_v = _guarded(torch, gpu, n, nsrc, off, pad, f64)
            assert off + pad == 0 or (src_v.stride(0) != n and tdst_v.stride(0) != nsrc)
            hip.transpose(src_v, tdst_v)
            want_full, want_v = _guarded(torch, gpu, n, nsrc, off, pad, f64)
            want_v.copy_(src.t())
            _same(torch, tdst_full, want_full, tag + ("transpose",))
            _same(torch, src_full, _guarded(torch, gpu, nsrc, n, off, pad, f64, src)[0], tag + ("the source was written",))
    torch.cuda.synchronize()
    # the 16-byte instance of the row-major kernel ran for even n (off = pad = 0, and off = 2 / pad = 8), the element instance
    # for everything else
    assert (vec_calls > 0) == (n % 2 == 0), (n, vec_calls)


SEG_ROWS = np.array([3, 0, 17, 29], np.int32)           # the list of test_gpu_transpose.py: an empty segment, a repeated source row
SEG_PTR = np.array([0, 3, 4, 4, 9], np.int32)
SEG_POS = np.array([5, 2, 39, 7, 1, 1, 8, 30, 0], np.int32)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_scatter_add_rows_both_instances_give_the_same_bits(crp, gpu, dt):
    """n = 24: lds = ldd = 24 on 16-byte-aligned pointers runs the 16-byte instance (VW = 2 / 4), ldd = 25 or a pointer one element
    off the element instance.  Which one runs follows from the alignment asserted here (csrc/row_kernels.hip: scatter_add_rows)."""
    import torch
    lib = crp.load()
    fn = lib.crp_scatter_add_rows_f64 if dt is np.float64 else lib.crp_scatter_add_rows_f32
    isz = np.dtype(dt).itemsize
    VW = 16 // isz
    tdt = torch.float64 if dt is np.float64 else torch.float32
    rng = np.random.default_rng(4)
    n, nsrc, ndst = 24, 40, 30
    src = _mantissa_full(rng, (nsrc, n), dt)
    dst = _mantissa_full(rng, (ndst, n), dt)
    want = dst.copy()
    for t, r in enumerate(SEG_ROWS):
        for k in range(SEG_PTR[t], SEG_PTR[t + 1]):
            want[r] = want[r] + src[SEG_POS[k]]
    assert want.dtype == dt and not np.array_equal(want, dst)
    d_rows, d_ptr, d_pos = (torch.from_numpy(a).to(gpu) for a in (SEG_ROWS, SEG_PTR, SEG_POS))
    census = []
    results = []
    # (ld of src, ld of dst, elements the src pointer is off, elements the dst pointer is off)
    for lds, ldd, soff, doff in ((24, 24, 0, 0), (24, 25, 0, 0), (24, 24, 0, 1), (24, 24, 1, 0), (25, 24, 0, 0), (24, 24 + VW, 0, 0)):
        s_flat = torch.full((soff + (nsrc + 2) * lds,), SENT, dtype=tdt, device=gpu)
        d_flat = torch.full((doff + (ndst + 2) * ldd,), SENT, dtype=tdt, device=gpu)
        w_flat = d_flat.clone()
        s_v = s_flat.as_strided((nsrc, n), (lds, 1), soff + lds)                  # one guard row above and below
        d_v = d_flat.as_strided((ndst, n), (ldd, 1), doff + ldd)
        s_v.copy_(torch.from_numpy(src))
        d_v.copy_(torch.from_numpy(dst))
        w_flat.as_strided((ndst, n), (ldd, 1), doff + ldd).copy_(torch.from_numpy(want))
        assert s_flat.data_ptr() % 16 == 0 and d_flat.data_ptr() % 16 == 0
        vec = n % VW == 0 and lds % VW == 0 and ldd % VW == 0 and (s_v.data_ptr() | d_v.data_ptr()) % 16 == 0
        census.append(vec)
        s_before = s_flat.clone()
        rc = fn(SEG_ROWS.size, n, d_rows.data_ptr(), d_ptr.data_ptr(), d_pos.data_ptr(), s_v.data_ptr(), lds, d_v.data_ptr(), ldd, None)
        torch.cuda.synchronize()
        tag = (dt.__name__, lds, ldd, soff, doff)
        assert rc == 0, tag
        _same(torch, d_flat, w_flat, tag)
        _same(torch, s_flat, s_before, tag + ("the source was written",))
        results.append(d_v.cpu().numpy())
    # the first and the last case are 16-byte aligned throughout (the last with guard columns between the rows): the vector instance;
    # each of the others breaks one condition: the element instance
    assert census == [True, False, False, False, False, True], census
    for got in results[1:]:
        assert np.array_equal(got.view(np.int64 if dt is np.float64 else np.int32), results[0].view(np.int64 if dt is np.float64 else np.int32))


def _past_cap_move(torch, gpu, hip_gather, hip_scatter, dt, nidx, n, pad, layout, work):
    """gather then scatter of nidx rows of n elements (layout 1: (n, ld) tensors) with `work` items > GRID_CAP each."""
    assert work > GRID_CAP, work
    rng = np.random.default_rng(nidx + n)
    tdt = torch.float64 if dt is np.float64 else torch.float32
    src = torch.from_numpy(_payload(rng, (nidx, n), dt)).to(gpu)
    perm = torch.from_numpy(rng.permutation(nidx).astype(np.int32)).to(gpu)
    shape = (nidx, n) if layout == 0 else (n, nidx)
    data = src if layout == 0 else src.t()
    src_full, src_v = _guarded(torch, gpu, shape[0], shape[1], 0, pad, tdt, data)
    dst_full, dst_v = _guarded(torch, gpu, shape[0], shape[1], 0, pad, tdt)
    assert max(src_full.numel(), dst_full.numel()) * src_full.element_size() < 20e6
    hip_gather(perm, src_v, dst_v, layout)
    want_full, want_v = _guarded(torch, gpu, shape[0], shape[1], 0, pad, tdt)
    want_v.copy_(src[perm.long()] if layout == 0 else src.t()[:, perm.long()])
    _same(torch, dst_full, want_full, (dt.__name__, layout, "gather"))
    out_full, out_v = _guarded(torch, gpu, shape[0], shape[1], 0, pad, tdt)
    hip_scatter(perm, dst_v, out_v, layout)                                    # scatter undoes the gather: out == src
    _same(torch, out_full, src_full, (dt.__name__, layout, "scatter"))
    return src_v, dst_v


def test_moves_past_the_grid_cap(crp, gpu):
    """gather / scatter of rows with more 16-byte pieces (row-major), elements (layout 1) or row groups (fp32) than one trip of the
    capped grid covers."""
    import torch
    from crp_spmm_amd import hip
    g64 = lambda r, s, d, layout: hip.gather_rows(r, s, d, layout=layout)
    s64 = lambda r, s, d, layout: hip.gather_rows(r, s, d, layout=layout, scatter=True)
    g32 = lambda r, s, d, layout: hip.gather_rows_f32(r, s, d, layout=layout)
    s32 = lambda r, s, d, layout: hip.scatter_rows_f32(r, s, d, layout=layout)
    # fp64, row-major: 4200 rows x 128 pieces of 16 bytes = 537 600; two guard columns keep ld even and every row 16-byte aligned
    sv, dv = _past_cap_move(torch, gpu, g64, s64, np.float64, 4200, 256, 2, 0, 4200 * 128)
    assert sv.stride(0) % 2 == 0 and (sv.data_ptr() | dv.data_ptr()) % 16 == 0, "the 16-byte instance was meant"
    # fp64, layout 1: one element per item, 4200 x 128
    _past_cap_move(torch, gpu, g64, s64, np.float64, 4200, 128, 3, 1, 4200 * 128)
    # fp32, row-major: 64 chunks of 16 bytes per row -> 64 lanes per row, 4 rows per workgroup: 8300 x 64 = 531 200 lanes
    sv, dv = _past_cap_move(torch, gpu, g32, s32, np.float32, 8300, 256, 4, 0, 8300 * 64)
    assert sv.stride(0) % 4 == 0 and (sv.data_ptr() | dv.data_ptr()) % 16 == 0, "the 16-byte instance was meant"
    # fp32, layout 1
    _past_cap_move(torch, gpu, g32, s32, np.float32, 8300, 64, 3, 1, 8300 * 64)


def test_scatter_add_rows_f64_past_the_grid_cap(crp, gpu):
    """4200 segments of 1 to 3 source rows at n = 256: 537 600 16-byte pieces."""
    import torch
    lib = crp.load()
    rng = np.random.default_rng(12)
    nseg, n, nsrc, ld = 4200, 256, 4000, 258
    assert nseg * (n // 2) > GRID_CAP
    lens = rng.integers(1, 4, size=nseg)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pos = rng.integers(0, nsrc, size=int(ptr[-1])).astype(np.int32)
    rows = rng.permutation(nseg).astype(np.int32)                               # distinct destination rows
    src = _mantissa_full(rng, (nsrc, n), np.float64)
    dst = _mantissa_full(rng, (nseg, n), np.float64)
    want = dst.copy()
    for t in range(3):                                                          # the t-th addition of every segment that has one
        segs = np.nonzero(lens > t)[0]
        want[rows[segs]] = want[rows[segs]] + src[pos[ptr[segs] + t]]
    d_src = torch.from_numpy(src).to(gpu)
    d_full, d_v = _guarded(torch, gpu, nseg, n, 0, ld - n, torch.float64, torch.from_numpy(dst))
    w_full, _w = _guarded(torch, gpu, nseg, n, 0, ld - n, torch.float64, torch.from_numpy(want))
    assert d_full.numel() * 8 < 20e6 and d_src.numel() * 8 < 20e6
    assert (d_src.data_ptr() | d_v.data_ptr()) % 16 == 0 and d_v.stride(0) % 2 == 0, "the 16-byte instance was meant"
    d_rows, d_ptr, d_pos = (torch.from_numpy(a).to(gpu) for a in (rows, ptr, pos))
    rc = lib.crp_scatter_add_rows_f64(nseg, n, d_rows.data_ptr(), d_ptr.data_ptr(), d_pos.data_ptr(), d_src.data_ptr(), n,
                                      d_v.data_ptr(), d_v.stride(0), None)
    torch.cuda.synchronize()
    assert rc == 0
    _same(torch, d_full, w_full, "scatter_add past the cap")


@pytest.mark.parametrize("dt,nseg,ln", [(np.float64, 3, 1100003), (np.float32, 3, 1100003), (np.float32, 2, 2200003)])
def test_sum_segments_past_the_grid_cap(crp, gpu, dt, nseg, ln):
    """A vector body plus an element tail.  fp64: 550 001 pieces of 16 bytes, past the cap.  fp32 at the same length has 275 000
    pieces -- one trip --, so a second fp32 case takes 2 200 003 elements in 2 segments: 550 000 pieces and a tail of 3 (the fp64
    source of 3 segments is 26 MB, every other buffer here stays below 20 MB)."""
    import torch
    lib = crp.load()
    fn = lib.crp_sum_segments_f64 if dt is np.float64 else lib.crp_sum_segments_f32
    VW = 16 // np.dtype(dt).itemsize
    assert ln % VW != 0 and (ln // VW > GRID_CAP or (dt is np.float32 and nseg == 3))
    rng = np.random.default_rng(ln)
    stride = ln + VW - ln % VW + VW                                             # a multiple of VW: the vector instance runs
    src = _mantissa_full(rng, (nseg - 1) * stride + ln, dt)
    want = src[:ln].copy()
    for j in range(1, nseg):
        want = want + src[j * stride:j * stride + ln]
    assert want.dtype == dt
    d_src = torch.from_numpy(src).to(gpu)
    d_out = torch.full((ln + 5,), SENT, dtype=d_src.dtype, device=gpu)
    assert d_src.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0 and stride % VW == 0
    rc = fn(nseg, ln, d_src.data_ptr(), stride, d_out.data_ptr(), None)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert rc == 0
    iv = np.int64 if dt is np.float64 else np.int32
    assert np.array_equal(got[:ln].view(iv), want.view(iv)) and (got[ln:] == SENT).all()


def test_gather_vals_past_the_grid_cap(crp, gpu):
    """crp_gather_vals_f64 / _f32_f64 at 600 011 entries, with and without a map."""
    import torch
    lib = crp.load()
    rng = np.random.default_rng(13)
    nn = 600011
    assert nn > GRID_CAP
    idx = rng.integers(0, nn, size=nn).astype(np.int32)
    d_idx = torch.from_numpy(idx).to(gpu)
    for dt, fn in ((np.float64, lib.crp_gather_vals_f64), (np.float32, lib.crp_gather_vals_f32_f64)):
        src = _mantissa_full(rng, nn, dt)
        d_src = torch.from_numpy(src).to(gpu)
        for mp, want in ((None, src.astype(np.float64)), (d_idx.data_ptr(), src[idx].astype(np.float64))):
            d_dst = torch.full((nn + 3,), SENT, dtype=torch.float64, device=gpu)
            rc = fn(nn, mp, d_src.data_ptr(), d_dst.data_ptr(), None)
            torch.cuda.synchronize()
            got = d_dst.cpu().numpy()
            assert rc == 0 and np.array_equal(got[:nn].view(np.int64), want.view(np.int64)) and (got[nn:] == SENT).all(), (dt.__name__, mp is None)
