"""GPU: the pattern and row kernels on operands past 2^31 elements (fp32) and past 2^32 bytes (fp64) -- tests/far_rows.py has the
arena, its layout and the case table, tests/test_far_rows_data.py shows on the CPU what a narrowed address would do, DESIGN.md 5u
the reasoning.

Every case of far_rows.CASES runs in both dtypes and in both instances (16-byte pieces: ld = 2^20, column offsets in fours;
single elements: ld = 2^20 + 1, odd offsets and widths), at two widths, and asserts
  1. the call on the arena views equals, bit for bit, the call on compact copies of the same alignment class;
  2. the compact result lies inside the family's existing bound against its existing reference (attention_ref, attention_bwd_ref,
     gat_ref, gatv2_ref, dropout_ref; the SDDMM's (n + 1) u S of DESIGN.md 5d; exact numpy for the row kernels, on
     integer data where a sum is formed);
  3. nothing else changed: everything outside columns [0, W) of the operand rows and the decoy rows is still the sentinel, and
     columns [0, W) are what they were, the outputs excepted.
Then the per-edge outputs indexed by out_pos * heads + h past index 2^31 (fp32 and the uint8 mask).

One arena is alive at a time: 16.25 GiB (float32), then 6.5 GiB (float64)."""
import functools

import numpy as np
import pytest

import attention_bwd_ref as B
import attention_ref as R
import dropout_ref as DR
import far_rows as FR
import gat_ref as G
import gatv2_ref as G2
import softmax_ref as SR

pytestmark = pytest.mark.gpu

SCALE, SLOPE = 0.25, 0.2
_ALIVE = []                              # the dtypes of the arenas alive: at most one


class Arena:
    """The arena of one dtype, the handles of its pattern, and the layout (ld) in use"""

    def __init__(self, gpu, dtype):
        import torch
        from crp_spmm_amd import hip
        assert not _ALIVE, "an arena is alive already: %s" % _ALIVE
        self.gpu, self.dtype, self.tier, self.tdt = gpu, dtype, FR.TIERS[dtype], getattr(torch, dtype)
        try:
            self.flat = torch.full((FR.arena_elems(dtype),), FR.SENT, dtype=self.tdt, device=gpu)
        except RuntimeError as e:
            pytest.fail("the %s arena of %d bytes could not be allocated: %s" % (dtype, FR.arena_bytes(dtype), str(e)[:300]))
        _ALIVE.append(dtype)
        self.inst, self.handles = None, []
        self.state = {}                  # forward results the backward cases read: computed once per (family, inst, w, ...)
        try:
            self.decoy_data = torch.from_numpy(FR.decoy_data(dtype)).to(gpu)
            pat = self.pat = FR.pattern(dtype)
            m = pat["m"]
            for make, ci in ((hip.CsrDev, pat["ci"]), (hip.CsrDev.from_transpose, pat["ci"]), (hip.CsrDev, pat["codes"])):
                self.handles.append(make(m, m, pat["rp"], ci, pat["val"]))
            self.A, self.At, self.A2 = self.handles
        except BaseException:            # the real error shows, and the next arena can still be made
            self.free()
            raise

    def free(self):
        import torch
        for h in self.handles:
            h.free()
        self.handles = []
        self.A = self.At = self.A2 = self.flat = self.decoy_data = None
        self.state.clear()
        torch.cuda.empty_cache()
        _ALIVE.remove(self.dtype)

    def rows2d(self, inst=None):
        import torch
        ld = FR.LD[inst or self.inst]
        return torch.as_strided(self.flat, (self.tier.rows, ld), (ld, 1))

    def use(self, inst):
        """switch the layout: what the old one holds in its first DECOY_W columns goes back to the sentinel, the decoy rows move"""
        if inst == self.inst:
            return
        if self.inst is not None:
            self.rows2d()[:, :FR.DECOY_W] = FR.SENT
            assert self._all_sentinel([self.flat]), "the arena is not all-sentinel between two layouts"
        self.inst = inst
        self.decoy().copy_(self.decoy_data)

    def decoy(self):
        return self.rows2d()[:FR.FAR, :FR.DECOY_W]

    def region(self):
        """columns [0, W) of the operand rows"""
        return self.rows2d()[self.tier.base:self.tier.base + self.tier.m, :FR.W]

    def view(self, p):
        return self.rows2d()[p.row0:p.row0 + p.rows, p.col:p.col + p.width]

    @staticmethod
    def _all_sentinel(parts):
        import torch
        ends = torch.stack([torch.stack(torch.aminmax(p)) for p in parts if p.numel()]).cpu().numpy()
        return bool((ends == FR.SENT).all())

    def sentinels_intact(self):
        """device-side reductions over everything but columns [0, W) of the operand rows and the decoy rows' data"""
        a, t = self.rows2d(), self.tier
        parts = [a[:, FR.DECOY_W:], a[FR.FAR:, FR.W:FR.DECOY_W], a[FR.FAR:t.base, :FR.W]]
        if self.inst == "vec":
            parts.append(self.flat[t.rows * FR.LD_VEC:])                   # (the slack of the odd ld)
        return self._all_sentinel(parts)


@pytest.fixture(scope="module")
def arena(request, gpu, crp):
    a = Arena(gpu, request.param)
    yield a
    a.free()


def _sent(arena, *shape):
    import torch
    return torch.full(shape, FR.SENT, dtype=arena.tdt, device=arena.gpu)


def _dev(arena, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(arena.gpu)


def _run(arena, inst, case, w, inputs, call):
    """The three assertions' common part.  inputs: name -> numpy array of every operand the call reads (an in/out operand's first
    contents among them); call(T) runs the call on the operands T (name -> tensor) and returns name -> tensor of everything it
    wrote.  Returns the compact run's results as numpy arrays."""
    import torch
    dtype = arena.dtype
    ops = FR.operands(case, dtype, w)
    placed = FR.place(dtype, inst, ops)
    arena.use(inst)
    region = arena.region()
    region.fill_(FR.SENT)
    far, compact = {}, {}
    for op in ops:
        v = arena.view(placed[op.name])
        ld, off = FR.compact_layout(dtype, inst, op.width)
        c = torch.as_strided(_sent(arena, op.rows * ld + off + 8), (op.rows, op.width), (ld, 1), storage_offset=off)
        if op.name in inputs:
            t = _dev(arena, inputs[op.name])
            assert t.shape == v.shape and t.dtype == arena.tdt, (op, t.shape, t.dtype)
            v.copy_(t)
            c.copy_(t)
        else:
            assert op.out, op
        assert (v.data_ptr() % 16 == 0) == (c.data_ptr() % 16 == 0) == (inst == "vec"), (op, "the alignment classes differ")
        far[op.name], compact[op.name] = v, c
    before, decoy_before = region.clone(), arena.decoy().clone()
    got_far = call(far)
    got = call(compact)
    torch.cuda.synchronize()
    what = (case.id, dtype, inst, w)
    for k in got:                                                          # 1. bit for bit
        assert got_far[k].shape == got[k].shape, what + (k,)
        assert torch.equal(got_far[k], got[k]), what + (k, "the call on the far rows differs from the call on the compact copies")
    after = region.clone()                                                 # 3. nothing else changed
    for op in ops:
        if op.out:
            p = placed[op.name]
            r0 = p.row0 - arena.tier.base
            after[r0:r0 + p.rows, p.col:p.col + p.width] = before[r0:r0 + p.rows, p.col:p.col + p.width]
    assert torch.equal(after, before), what + ("columns [0, W) of the operand rows changed outside the outputs",)
    assert torch.equal(arena.decoy(), decoy_before), what + ("the decoy rows changed",)
    assert arena.sentinels_intact(), what + ("a sentinel outside the operands was overwritten",)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _rng(*key):
    """a generator seeded by the key's text: the same data in every process"""
    return np.random.default_rng([ord(c) for c in repr(key)])


def _inside(ratios, what):
    print("%s: worst |got - ref| / bound  %s" % (what, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    assert all(v <= 1 for v in ratios.values()), (what, ratios)


# ---- SDDMM ------------------------------------------------------------------------------------------------------------------

def _sddmm(crp, arena, inst, case, w):
    import torch
    dtype, pat = arena.dtype, arena.pat
    m, nnz = pat["m"], pat["ci"].size
    rng = _rng("sddmm", dtype, w)
    X, Y0, Y1 = (FR.row_data(rng, m, w, dtype) for _ in range(3))
    two = case.kw["sources"] == 2
    handle = arena.A2 if two else arena.A

    def call(T):
        out = _sent(arena, nnz)
        handle.sddmm(T["X"], T["Y0"], Y1=T.get("Y1"), out=out)
        return dict(out=out)
    got = _run(arena, inst, case, w, dict(X=X, Y0=Y0, Y1=Y1) if two else dict(X=X, Y0=Y0), call)
    codes = pat["codes"] if two else pat["ci"]
    ref, S = FR.dot_reference(pat["rp"], np.where(codes < 0, m + ~codes, codes), X, np.concatenate([Y0, Y1]))
    _inside({"out": FR.worst_ratio(got["out"], ref, (w + 1) * SR.U[np.dtype(dtype)] * S)}, (case.id, dtype, inst, w))


# ---- the fused attention ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _attention_data(dtype, w, H):
    """(Q, K, V, dO, the reference of every head)"""
    pat = FR.pattern(dtype)
    rng = _rng("attention", dtype, w, H)
    ops = tuple(FR.row_data(rng, pat["m"], H * w, dtype) for _ in range(4))
    bias = pat["val"].astype(dtype)
    heads = [tuple(np.ascontiguousarray(x[:, h * w:(h + 1) * w]) for x in ops) for h in range(H)]
    return ops + ([B.reference(pat["rp"], pat["ci"], q, k, v, do, SCALE, bias, ncol=pat["m"]) for q, k, v, do in heads],)


def _vec(arena, rows, H):
    return _sent(arena, rows) if H == 1 else _sent(arena, rows, H)


def _attention_state(arena, w, H):
    """(O, lse, delta) of the forward and the row side on contiguous operands: what the backward cases read"""
    import torch
    key = ("attention", w, H)
    if key not in arena.state:
        Q, K, V, dO, _ = _attention_data(arena.dtype, w, H)
        Q, K, V, dO = (_dev(arena, x) for x in (Q, K, V, dO))
        lse = _vec(arena, Q.shape[0], H)
        O = arena.A.attention(Q, K, V, scale=SCALE, bias=True, lse=lse, heads=H)
        _, delta = arena.A.attention_bwd_q(Q, K, V, O, dO, lse, scale=SCALE, bias=True, heads=H)
        torch.cuda.synchronize()
        arena.state[key] = (O.cpu().numpy(), lse, delta)
    return arena.state[key]


def _attention(crp, arena, inst, case, w):
    dtype, pat, H = arena.dtype, arena.pat, case.kw["heads"]
    m, nnz = pat["m"], pat["ci"].size
    Q, K, V, dO, refs = _attention_data(dtype, w, H)
    O, lse, delta = _attention_state(arena, w, H)
    what = (case.id, dtype, inst, w)
    sv = lambda h: slice(h * w, (h + 1) * w)
    if case.call == "attention":
        def call(T):
            l, p = _vec(arena, m, H), _vec(arena, nnz, H)
            arena.A.attention(T["Q"], T["K"], T["V"], scale=SCALE, bias=True, out=T["O"], lse=l, p_out=p, heads=H)
            return dict(O=T["O"], lse=l, p=p)
        got = _run(arena, inst, case, w, dict(Q=Q, K=K, V=V), call)
        gl, gp = got["lse"].reshape(m, H), got["p"].reshape(nnz, H)
        for h in range(H):
            ref = refs[h]["fwd"]
            live = np.isfinite(ref["lse"].astype(np.float64))
            assert np.isfinite(got["O"]).all() and np.isfinite(gp).all(), what
            assert np.array_equal(np.isfinite(gl[:, h]), live) and (gl[~live, h] == -np.inf).all(), what + ("lse of the empty rows",)
            _inside({"O": SR.worst(got["O"][:, sv(h)].ravel(), ref["O"].ravel(), R.bound_O(ref, dtype).ravel())[0],
                     "p_out": SR.worst(gp[:, h], ref["p"], R.bound_p(ref, dtype))[0],
                     "lse": SR.worst(gl[live, h], ref["lse"][live], R.bound_lse(ref, dtype)[live])[0]}, what + (h,))
    elif case.call == "attention_bwd_q":
        def call(T):
            d, ds = _vec(arena, m, H), _vec(arena, nnz, H)
            arena.A.attention_bwd_q(T["Q"], T["K"], T["V"], T["O"], T["dO"], lse, scale=SCALE, bias=True, dQ=T["dQ"], delta=d, ds_out=ds,
                                    heads=H)
            return dict(dQ=T["dQ"], delta=d, ds=ds)
        got = _run(arena, inst, case, w, dict(Q=Q, K=K, V=V, O=O, dO=dO), call)
        for h in range(H):
            _inside(B.ratios(dict(dQ=got["dQ"][:, sv(h)], delta=got["delta"].reshape(m, H)[:, h], ds=got["ds"].reshape(nnz, H)[:, h]), refs[h],
                             dtype), what + (h,))
    else:
        def call(T):
            arena.At.attention_bwd_kv(T["K"], T["V"], T["Q"], T["dO"], lse, delta, scale=SCALE, bias=True, dK=T["dK"], dV=T["dV"], heads=H)
            return dict(dK=T["dK"], dV=T["dV"])
        got = _run(arena, inst, case, w, dict(K=K, V=V, Q=Q, dO=dO), call)
        for h in range(H):
            _inside(B.ratios(dict(dK=got["dK"][:, sv(h)], dV=got["dV"][:, sv(h)]), refs[h], dtype), what + (h,))


# ---- GAT and GATv2 ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gat_data(fam, dtype, w, H, drop):
    """the operands and name -> (reference, bound): (el, er, V, dO, ref) or (XT, XS, a, dO, ref)"""
    pat = FR.pattern(dtype)
    m, rp, ci = pat["m"], pat["rp"], pat["ci"]
    rng = _rng(fam, dtype, w, H)
    if fam == "gat":
        el, er = FR.row_data(rng, m, H, dtype), FR.row_data(rng, m, H, dtype)
        V, dO = FR.row_data(rng, m, H * w, dtype), FR.row_data(rng, m, H * w, dtype)
        ref = DR.gat_reference(rp, ci, el, er, V, SLOPE, drop, FR.SEED, None, dO) if drop else G.reference(rp, ci, el, er, V, SLOPE, None, dO)
        return el, er, V, dO, ref
    XT, XS, dO = (FR.row_data(rng, m, H * w, dtype) for _ in range(3))
    a = (rng.standard_normal((H, w)) / np.sqrt(w)).astype(dtype)
    ref = DR.gatv2_reference(rp, ci, XT, XS, a, SLOPE, drop, FR.SEED, None, dO) if drop else G2.reference(rp, ci, XT, XS, a, SLOPE, None, dO)
    return XT, XS, a, dO, ref


def _gat(crp, arena, inst, case, w):
    import torch
    dtype, pat, H, drop = arena.dtype, arena.pat, case.kw["heads"], case.kw["dropout"]
    m, nnz = pat["m"], pat["ci"].size
    kw = dict(slope=SLOPE, heads=H, dropout=drop, seed=FR.SEED if drop else 0)
    el, er, V, dO, ref = _gat_data("gat", dtype, w, H, drop)
    key = ("gat", w, H, drop)
    if key not in arena.state:
        t = [_dev(arena, x) for x in (el, er, V, dO)]
        lse = _sent(arena, m, H)
        O = arena.A.gat_attention(t[0], t[1], t[2], lse=lse, **kw)
        _, delta = arena.A.gat_attention_bwd_row(t[0], t[1], t[2], O, t[3], lse, **kw)
        torch.cuda.synchronize()
        arena.state[key] = (O.cpu().numpy(), lse, delta)
    O, lse, delta = arena.state[key]
    if case.call == "gat_attention":
        def call(T):
            l, p = _sent(arena, m, H), _sent(arena, nnz, H)
            arena.A.gat_attention(T["el"], T["er"], T["V"], out=T["O"], lse=l, p_out=p, **kw)
            return dict(O=T["O"], lse=l, p=p)
        got = _run(arena, inst, case, w, dict(el=el, er=er, V=V), call)
    elif case.call == "gat_attention_bwd_row":
        def call(T):
            d, ds = _sent(arena, m, H), _sent(arena, nnz, H)
            arena.A.gat_attention_bwd_row(T["el"], T["er"], T["V"], T["O"], T["dO"], lse, d_el=T["d_el"], delta=d, ds_out=ds, **kw)
            return dict(d_el=T["d_el"], delta=d, ds=ds)
        got = _run(arena, inst, case, w, dict(el=el, er=er, V=V, O=O, dO=dO), call)
    else:
        def call(T):
            arena.At.gat_attention_bwd_col(T["er"], T["V"], T["el"], T["dO"], lse, delta, d_er=T["d_er"], dV=T["dV"], **kw)
            return dict(d_er=T["d_er"], dV=T["dV"])
        got = _run(arena, inst, case, w, dict(er=er, V=V, el=el, dO=dO), call)
    _inside(G.ratios(got, ref), (case.id, dtype, inst, w))


def _gatv2(crp, arena, inst, case, w):
    import torch
    dtype, pat, H, drop = arena.dtype, arena.pat, case.kw["heads"], case.kw["dropout"]
    m, nnz = pat["m"], pat["ci"].size
    kw = dict(slope=SLOPE, heads=H, dropout=drop, seed=FR.SEED if drop else 0)
    XT, XS, a, dO, ref = _gat_data("gatv2", dtype, w, H, drop)
    ad = _dev(arena, a)
    key = ("gatv2", w, H, drop)
    if key not in arena.state:
        t = [_dev(arena, x) for x in (XT, XS, dO)]
        lse = _sent(arena, m, H)
        O = arena.A.gatv2_attention(t[0], t[1], ad, lse=lse, **kw)
        _, _, delta = arena.A.gatv2_attention_bwd_row(t[0], t[1], ad, O, t[2], lse, **kw)
        torch.cuda.synchronize()
        arena.state[key] = (O.cpu().numpy(), lse, delta)
    O, lse, delta = arena.state[key]
    if case.call == "gatv2_attention":
        def call(T):
            l, p = _sent(arena, m, H), _sent(arena, nnz, H)
            arena.A.gatv2_attention(T["XT"], T["XS"], ad, out=T["O"], lse=l, p_out=p, **kw)
            return dict(O=T["O"], lse=l, p=p)
        got = _run(arena, inst, case, w, dict(XT=XT, XS=XS), call)
    elif case.call == "gatv2_attention_bwd_row":
        def call(T):
            d, ds = _sent(arena, m, H), _sent(arena, nnz, H)
            arena.A.gatv2_attention_bwd_row(T["XT"], T["XS"], ad, T["O"], T["dO"], lse, dXT=T["dXT"], da_part=T["da_part"], delta=d, ds_out=ds,
                                            **kw)
            return dict(dXT=T["dXT"], da_part=T["da_part"], delta=d, ds=ds)
        got = _run(arena, inst, case, w, dict(XT=XT, XS=XS, O=O, dO=dO), call)
    else:
        def call(T):
            arena.At.gatv2_attention_bwd_col(T["XS"], T["XT"], ad, T["dO"], lse, delta, dXS=T["dXS"], **kw)
            return dict(dXS=T["dXS"])
        got = _run(arena, inst, case, w, dict(XS=XS, XT=XT, dO=dO), call)
    _inside(G2.ratios(got, ref), (case.id, dtype, inst, w))


# ---- the row kernels ----------------------------------------------------------------------------------------------------------

def _rows(crp, arena, inst, case, w):
    from crp_spmm_amd import hip
    lib = crp.load()
    dtype, m = arena.dtype, arena.tier.m
    f32 = dtype == "float32"
    sfx = "f32" if f32 else "f64"
    rng = _rng("rows", case.id, dtype, w)
    perm, seg_row, seg_ptr, seg_pos = FR.move_lists(m)
    c = case.call
    if c in ("gather_rows", "scatter_rows"):
        layout, scatter = case.kw["layout"], c == "scatter_rows"
        src = FR.row_data(rng, m, w, dtype)
        idx = perm if layout == 0 else rng.permutation(w).astype(np.int32)          # layout 1: the arena rows are the columns
        ridx = _dev(arena, idx)
        want = np.empty_like(src)
        if layout == 0:
            if scatter:
                want[idx] = src
            else:
                want = src[idx]
        elif scatter:
            want[:, idx] = src
        else:
            want = src[:, idx]

        def call(T):
            if f32:
                (hip.scatter_rows_f32 if scatter else hip.gather_rows_f32)(ridx, T["src"], T["dst"], layout=layout)
            else:
                hip.gather_rows(ridx, T["src"], T["dst"], layout=layout, scatter=scatter)
            return dict(dst=T["dst"])
        got = _run(arena, inst, case, w, dict(src=src), call)["dst"]
    elif c == "transpose":
        src = FR.row_data(rng, m, w, dtype) if case.kw["far"] == "src" else FR.row_data(rng, w, m, dtype)
        want = np.ascontiguousarray(src.T)

        def call(T):
            (hip.transpose_f32 if f32 else hip.transpose)(T["src"], T["dst"])
            return dict(dst=T["dst"])
        got = _run(arena, inst, case, w, dict(src=src), call)["dst"]
    elif c == "scatter_add_rows":
        src, dst = FR.row_data(rng, m, w, dtype, integers=True), FR.row_data(rng, m, w, dtype, integers=True)
        want = dst.astype(np.float64)
        np.add.at(want, np.repeat(seg_row, np.diff(seg_ptr)), src[seg_pos].astype(np.float64))
        want = want.astype(dtype)
        lists = [_dev(arena, x) for x in (seg_row, seg_ptr, seg_pos)]
        fn = getattr(lib, "crp_scatter_add_rows_" + sfx)

        def call(T):
            s, d = T["src"], T["dst"]
            rc = fn(seg_row.size, w, lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), s.data_ptr(), s.stride(0), d.data_ptr(),
                    d.stride(0), hip._stream(d))
            assert rc == 0, rc
            return dict(dst=d)
        got = _run(arena, inst, case, w, dict(src=src, dst=dst), call)["dst"]
    else:
        src = FR.row_data(rng, m, w, dtype, integers=True)
        want = src.astype(np.float64).sum(axis=0).astype(dtype)                      # (exact: integers)
        fn = getattr(lib, "crp_sum_segments_" + sfx)

        def call(T):
            s = T["src"]
            if c == "col_sum":
                return dict(out=hip.col_sum(s))
            out = _sent(arena, w)
            rc = fn(m, w, s.data_ptr(), s.stride(0), out.data_ptr(), hip._stream(out))          # the arena rows are the segments
            assert rc == 0, rc
            return dict(out=out)
        got = _run(arena, inst, case, w, dict(src=src), call)["out"]
    assert got.dtype == want.dtype and np.array_equal(got, want), (case.id, dtype, inst, w, "differs from numpy")


FAMILIES = dict(sddmm=_sddmm, attention=_attention, gat=_gat, gatv2=_gatv2, rows=_rows)


@pytest.mark.parametrize("case_id", [c.id for c in FR.CASES])
@pytest.mark.parametrize("inst", FR.INSTANCES)
@pytest.mark.parametrize("arena", FR.DTYPES, indirect=True)
def test_far_rows(crp, gpu, arena, inst, case_id):
    case = FR.CASE_BY_ID[case_id]
    for w in FR.WIDTHS[inst]:
        FAMILIES[case.family](crp, arena, inst, case, w)


# ---- the per-edge index times heads -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", FR.POS_CALLS)
@pytest.mark.parametrize("arena", ["float32"], indirect=True)
def test_edge_index_times_heads_past_2_31(crp, gpu, arena, call):
    """out_pos rows up to 2^28 + 63 of a contiguous (2^28 + 64, 8) view that starts 2^31 elements (the mask: bytes) into the arena:
    index out_pos * 8 + h reaches 2^31.  Against the call without out_pos, permuted; the float64 outputs would need 16 GiB more."""
    import torch
    H, w = FR.POS_HEADS, 8
    pat = arena.pat
    m, nnz = pat["m"], pat["ci"].size
    arena.use(arena.inst or "vec")
    pos_np = FR.out_positions(nnz)
    pos = _dev(arena, pos_np)
    idx = pos.long()
    store = arena.flat.view(torch.uint8) if call == "dropout_mask" else arena.flat
    view = store[FR.POS_BASE:FR.POS_BASE + FR.POS_ROWS * H].view(FR.POS_ROWS, H)
    assert view.is_contiguous() and view.data_ptr() == arena.flat.data_ptr() + FR.POS_BASE * (1 if call == "dropout_mask" else 4)
    region_before, decoy_before = arena.region().clone(), arena.decoy().clone()
    saved = view[idx].clone()
    rng = _rng("pos", call)
    same = {}
    if call == "attention.p_out":
        Q, K, V = (_dev(arena, FR.row_data(rng, m, H * w, "float32")) for _ in range(3))
        want = _sent(arena, nnz, H)
        O1 = arena.A.attention(Q, K, V, scale=SCALE, bias=True, p_out=want, heads=H)
        O2 = arena.A.attention(Q, K, V, scale=SCALE, bias=True, p_out=view, out_pos=pos, heads=H)
        same = dict(O=(O1, O2))
    elif call == "dropout_mask":
        want = arena.A.dropout_mask(H, FR.DROP, FR.SEED)
        arena.A.dropout_mask(H, FR.DROP, FR.SEED, out=view, out_pos=pos)
        assert np.array_equal(want.cpu().numpy().astype(bool), DR.mask_csr(pat["rp"], pat["ci"], H, FR.DROP, FR.SEED))
    else:
        el, er = (_dev(arena, FR.row_data(rng, m, H, "float32")) for _ in range(2))
        V, dO = (_dev(arena, FR.row_data(rng, m, H * w, "float32")) for _ in range(2))
        lse, want = _sent(arena, m, H), _sent(arena, nnz, H)
        if call == "gat_attention.p_out":
            O1 = arena.A.gat_attention(el, er, V, slope=SLOPE, p_out=want, heads=H)
            O2 = arena.A.gat_attention(el, er, V, slope=SLOPE, p_out=view, out_pos=pos, heads=H)
            same = dict(O=(O1, O2))
        else:
            O = arena.A.gat_attention(el, er, V, slope=SLOPE, lse=lse, heads=H)
            e1, d1 = arena.A.gat_attention_bwd_row(el, er, V, O, dO, lse, slope=SLOPE, ds_out=want, heads=H)
            e2, d2 = arena.A.gat_attention_bwd_row(el, er, V, O, dO, lse, slope=SLOPE, ds_out=view, out_pos=pos, heads=H)
            same = dict(d_el=(e1, e2), delta=(d1, d2))
    torch.cuda.synchronize()
    got = view[idx]
    view[idx] = saved                                                      # (before any assertion: the arena stays as it was)
    torch.cuda.synchronize()
    assert not bool((want == FR.SENT).any()) and torch.equal(got, want), (call, "the rows out_pos names differ from the call without it")
    for k, (x, y) in same.items():
        assert torch.equal(x, y), (call, k)
    assert torch.equal(arena.region(), region_before) and torch.equal(arena.decoy(), decoy_before), (call, "something else was written")
    assert arena.sentinels_intact(), (call, "a sentinel outside the rows out_pos names was overwritten")


@pytest.mark.parametrize("arena", FR.DTYPES, indirect=True)
def test_the_sentinel_reductions_see_one_changed_element(gpu, arena):
    """one element changed in each part the reductions cover -- first and last of the wide part, the strip beside the decoy data,
    the rows between the decoy rows and the operands, the last operand row past column 2 W -- is seen, and put back"""
    arena.use(arena.inst or "vec")
    assert arena.sentinels_intact()
    a, t = arena.rows2d(), arena.tier
    for r, c in ((0, FR.DECOY_W), (t.rows - 1, FR.LD[arena.inst] - 1), (FR.FAR, FR.W), (t.base - 1, 0), (t.base + t.m - 1, FR.DECOY_W + 5)):
        a[r, c] = 1.0
        assert not arena.sentinels_intact(), (r, c)
        a[r, c] = FR.SENT
    assert arena.sentinels_intact()
