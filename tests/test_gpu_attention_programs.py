"""GPU: one handle pair and one row engine run through the seeded programs of tests/attention_programs.py -- the multi-head, GAT,
GATv2 and dropout calls in sequence, every step checked against the model.

The runners are those of tests/test_gpu_call_programs.py in outline (its ``Streams``, its snapshots and its failure report are
reused): every output goes into its own NaN-filled tensor allocated before the first step (0xFF-filled for the uint8 masks), the
steps alternate between the default stream and two non-blocking ones, ordered by events only, and after ONE synchronisation
every output is compared.

Handle programs, every step:

    a.  bit for bit the same call on a FRESH pair of handles made from the model's current values and carrying the model's current
        row maps (the backward steps read O, lse and delta of the forward on that fresh pair, so both runs read the same bits);
        everything finite but the lse of empty rows
    b.  ``mask`` steps equal attention_programs.mask_of -- numpy's Philox under the key csrc/dropout.h documents, never the
        library; for every dropout step the fresh pair's ``dropout_mask`` at the step's (heads, rate, seed) equals it too, which
        with a. and the generator's sensitivity rule (the masks under the current and the previous row map differ in a quarter of
        their entries) pins the bits the step itself drew
    c.  inside the derived bounds of attention_ref / attention_bwd_ref per head, gat_ref, gatv2_ref, or under dropout
        dropout_ref.gat_reference / gatv2_reference with ``rowmap=`` and ``codes=`` -- wherever attention_programs.bounded says so
    d.  padding columns, rows the handle's row map does not name and positions out_pos does not name (all heads' columns of them)
        still hold their fill

    after every step the queries equal the model's; after the last one a variant-1 fp64 product on each handle equals the model's.

Engine programs (RpSpmm), one runner class for one rank in this process (comm.SelfComm) and for the ranks of
tests/gpu_dist_attention_programs_worker.py (comm.TorchComm): exec, exec_t and sddmm exactly under an E set (the int64 model has one
bit pattern whatever the order of the cross-rank sum) and by the fp64 / fp32 bounds otherwise; attn, gat, gatv2, the softmax and
dQ / ds_out of attn_bwd bit for bit this rank's slice of the handle calls on a fresh pair of handles of the FULL matrix at the
model's current values; dK and dV bit for bit at one rank and inside attention_bwd_ref's per-head bounds at several.

A failure names the program's seed, the step's index and the step, and prints the prefix up to it as a literal.  Each test prints
its device time, its wall time and the worst error-to-bound ratios seen so far.
"""
import time

import numpy as np
import pytest

import attention_bwd_ref as BR
import attention_programs as AP
import attention_ref as R
import call_programs as CP
import dropout_ref as DR
import gat_ref as G
import gatv2_ref as G2
import softmax_ref as SR
import test_gpu_call_programs as T1

pytestmark = pytest.mark.gpu

NP, WORST = T1.NP, T1.WORST
Streams, _bits, _note = T1.Streams, T1._bits, T1._note
FILL8 = 0xFF                            # what a uint8 mask holds where nothing was written
COUNTS = {"handle": [0, 0, 0], "engine": [0, 0, 0]}          # steps, compared bit for bit, held to bounds


class Snap:
    """what the model held when a step was issued"""

    def __init__(self, kind, val, cur, map_a, map_t, data):
        self.kind, self.val, self.cur, self.map_a, self.map_t = kind, val, cur, map_a, map_t
        self.rm_a, self.rows_a = data.rowmap("A", map_a)
        self.rm_t, self.rows_t = data.rowmap("T", map_t)


def _same_bits(got, fresh, what):
    for name in fresh:
        a, b = _bits(got[name]), _bits(fresh[name])
        assert a.shape == b.shape and np.array_equal(a, b), \
            (what, "%s differs from the same call on fresh handles at %d entries" % (name, int((a != b).sum()) if a.shape == b.shape else -1))


def _unwritten(a):
    return (a == FILL8) if a.dtype == np.uint8 else np.isnan(a)


def _named(out, idx, what, which):
    """the rows of an output that a row map or out_pos names; every other row must still hold its fill, in every column"""
    if idx is None:
        return out
    rest = np.ones(out.shape[0], bool)
    rest[idx] = False
    assert _unwritten(out[rest]).all(), (what, "a %s was written" % which)
    return out[idx]


def _ratios(tag, dtype, ratios, what):
    for k, w in ratios.items():
        _note("%s %s %s" % (tag, k, dtype), w)
        assert w <= 1, (what, "bound missed", k, w)


class Stranded(AssertionError):
    """a failure while the steps were being issued: at several ranks the peers are left inside the step's exchange"""


class Entry:
    """one call step: make() -> its outputs, pre(fA, fAt) -> what a backward reads (from the fresh pair), launch(A, At, outs, pre),
    check(outs as numpy, what), and for a dropout step (handle, heads, rate, seed)"""

    def __init__(self, make, launch, check, pre=None, bounded=False):
        self.make, self.launch, self.check, self.pre, self.bounded = make, launch, check, pre, bounded
        self.outs, self.fresh, self.given = make(), None, None


# ---- the device handles ----------------------------------------------------------------------------------------------------------

class HandleRun(T1.Base):
    def __init__(self, prog, gpu):
        self.prog = prog
        pat, data, self.model = AP.handle_setup(prog)
        super().__init__(gpu, data)
        self.vals_dev = [self.dev(vs.val) for vs in data.sets]
        self.pos_dev = self.dev(data.out_pos)
        self.pos_np = data.out_pos.astype(np.int64)
        self.live = np.diff(pat.rp) > 0

    def handles(self, snap):
        from crp_spmm_amd import hip
        pat = self.pat
        A = hip.CsrDev(pat.m, pat.ncol0, pat.rp, pat.codes, snap.val)
        At = hip.CsrDev.from_transpose(pat.m, pat.k, pat.rp, pat.gcol, snap.val)
        if snap.rm_a is not None:
            A.set_rowmap(snap.rm_a, snap.rows_a)
        if snap.rm_t is not None:
            At.set_rowmap(snap.rm_t, snap.rows_t)
        return A, At

    def snapshot(self):
        m = self.model
        return Snap(m.values.kind, m.values.val, m.cur, m.map["A"], m.map["T"], self.data)

    # -- operands: a row per row of A placed by A's map, a row per column of A split by source (A) or placed by A^T's map
    def placed(self, key, a, dtype, rm, rows):
        def make():
            if rm is None:
                return self.dev(a.astype(NP[dtype]))
            full = np.full((rows,) + a.shape[1:], np.nan, NP[dtype])
            full[rm] = a
            return self.dev(full)
        return self.cached((key, dtype, a.shape, id(rm)), make)

    def by_a(self, key, a, dtype, snap):
        return self.placed(key, a, dtype, snap.rm_a, snap.rows_a)

    def by_t(self, key, a, dtype, snap):
        return self.placed(key + "/T", a, dtype, snap.rm_t, snap.rows_t)

    def sources(self, key, a, dtype):
        return self.cached((key + "/src", dtype, a.shape), lambda: self.split(a, dtype))

    def plain(self, key, a, dtype):
        return self.cached((key + "/plain", dtype, a.shape), lambda: self.dev(np.ascontiguousarray(a).astype(NP[dtype])))

    def vec(self, t, H):
        return t.view(-1) if H == 1 else t

    def back(self, t, snap):
        """rows of A's order out of a tensor that A's map placed"""
        if snap.rm_a is None:
            return t
        idx = self.cached(("idx", id(snap.rm_a)), lambda: self.dev(snap.rm_a.astype(np.int64)))
        return t.index_select(0, idx).contiguous()

    def pos(self, use_pos):
        return (self.pos_dev, self.pos_np) if use_pos else (None, None)

    def per_nnz(self, H, dtype, use_pos):
        n = self.pat.gcol.size + (CP.OUT_EXTRA if use_pos else 0)
        return self.nan((n, H), dtype)

    def finite(self, got, what, lse=()):
        for k, v in got.items():
            if k in lse:
                live = self.live
                assert np.isfinite(v[live]).all() and (v[~live] == -np.inf).all(), (what, k, "lse of empty rows")
            else:
                assert np.isfinite(v).all(), (what, k, "non-finite output")

    def build(self, step, snap):
        k = step[0]
        if k in AP.ATTN:
            return self._attention(step, snap)
        if k in AP.GATS:
            return self._gat(step, snap, k.startswith("gatv2"))
        return getattr(self, "_" + k)(step, snap)

    # -- the fused attention with heads
    def _attention(self, step, snap):
        kind, _, dtype, bias, H, widx = step[:6]
        use_pos = step[6] if kind != "bwd_kv" else False
        dk, dv = CP.ATTN_WIDTHS[widx]
        nk, nv = H * dk, H * dv
        dt = NP[dtype]
        pat, data = self.pat, self.data
        scale = 1.0 / np.sqrt(dk)
        Q, dO = self.by_a("Q", data.Q[:, :nk], dtype, snap), self.by_a("dO", data.dO[:, :nv], dtype, snap)
        (K0, K1), (V0, V1) = self.sources("K", data.K[:, :nk], dtype), self.sources("V", data.V[:, :nv], dtype)
        posd, posn = self.pos(use_pos)
        bounded = AP.bounded(step, self.model, self.prog.two_source)
        ra, rt = snap.rows_a, snap.rows_t

        def forward(A, O, lse, p=None):
            A.attention(Q, K0, V0, K1=K1, V1=V1, scale=scale, bias=bias, out=O, lse=self.vec(lse, H), p_out=None if p is None else self.vec(p, H),
                        out_pos=posd if p is not None else None, heads=H)

        def refs(bwd):
            key = ("aref", bwd, dtype, bias, H, widx, snap.cur if bias else None)
            def make():
                out = []
                for h in range(H):
                    a = (pat.rp, pat.gcol, data.Q[:, h * dk:(h + 1) * dk].astype(dt), data.K[:, h * dk:(h + 1) * dk].astype(dt),
                         data.V[:, h * dv:(h + 1) * dv].astype(dt))
                    b = snap.val.astype(dt) if bias else None
                    out.append(BR.reference(*a, data.dO[:, h * dv:(h + 1) * dv].astype(dt), dt(scale), b, ncol=pat.k) if bwd
                               else R.reference(*a, dt(scale), b))
                return out
            return self.cached(key, make)

        if kind == "attn":
            make = lambda: {"O": self.nan((ra, nv + 3), dtype), "lse": self.nan((ra, H), dtype), "p": self.per_nnz(H, dtype, use_pos)}
            launch = lambda A, At, o, pre: forward(A, o["O"][:, :nv], o["lse"], o["p"])

            def check(o, what):
                assert np.isnan(o["O"][:, nv:]).all(), (what, "padding written")
                got = {"O": _named(o["O"][:, :nv], snap.rm_a, what, "row that the row map does not name"),
                       "lse": _named(o["lse"], snap.rm_a, what, "row that the row map does not name"),
                       "p": _named(o["p"], posn, what, "position that out_pos does not name")}
                self.finite(got, what, lse=("lse",))
                if bounded:
                    for h, ref in enumerate(refs(False)):
                        live = self.live
                        _ratios("attention", dtype, {"O": R.worst(got["O"][:, h * dv:(h + 1) * dv].ravel(), ref["O"].ravel(), R.bound_O(ref, dt).ravel())[0],
                                                     "p_out": R.worst(got["p"][:, h], ref["p"], R.bound_p(ref, dt))[0],
                                                     "lse": R.worst(got["lse"][live, h], ref["lse"][live], R.bound_lse(ref, dt)[live])[0]}, what)
            return Entry(make, launch, check, None, bounded)

        def pre(fA, fAt):
            O, lse = self.nan((ra, nv), dtype), self.nan((ra, H), dtype)
            forward(fA, O, lse)
            given = {"O": O, "lse": lse}
            if kind == "bwd_kv":
                delta = self.nan((ra, H), dtype)
                fA.attention_bwd_q(Q, K0, V0, O, dO, self.vec(lse, H), K1=K1, V1=V1, scale=scale, bias=bias, delta=self.vec(delta, H), heads=H)
                given = {"lse": self.back(lse, snap), "delta": self.back(delta, snap)}
            return given

        if kind == "bwd_q":
            make = lambda: {"dQ": self.nan((ra, nk + 3), dtype), "delta": self.nan((ra, H), dtype), "ds": self.per_nnz(H, dtype, use_pos)}

            def launch(A, At, o, given):
                A.attention_bwd_q(Q, K0, V0, given["O"], dO, self.vec(given["lse"], H), K1=K1, V1=V1, scale=scale, bias=bias, dQ=o["dQ"][:, :nk],
                                  delta=self.vec(o["delta"], H), ds_out=self.vec(o["ds"], H), out_pos=posd, heads=H)

            def check(o, what):
                assert np.isnan(o["dQ"][:, nk:]).all(), (what, "padding written")
                got = {"dQ": _named(o["dQ"][:, :nk], snap.rm_a, what, "row that the row map does not name"),
                       "delta": _named(o["delta"], snap.rm_a, what, "row that the row map does not name"),
                       "ds": _named(o["ds"], posn, what, "position that out_pos does not name")}
                self.finite(got, what)
                if bounded:
                    for h, ref in enumerate(refs(True)):
                        _ratios("attention_bwd", dtype, BR.ratios({"dQ": got["dQ"][:, h * dk:(h + 1) * dk], "delta": got["delta"][:, h],
                                                                  "ds": got["ds"][:, h]}, ref, dt), what)
            return Entry(make, launch, check, pre, bounded)

        # bwd_kv on the single-source handle of A^T: K and V a row per row of that handle, Q and dO a row per row of A
        Kt, Vt = self.by_t("K", data.K[:, :nk], dtype, snap), self.by_t("V", data.V[:, :nv], dtype, snap)
        Qp, dOp = self.plain("Q", data.Q[:, :nk], dtype), self.plain("dO", data.dO[:, :nv], dtype)
        make = lambda: {"dK": self.nan((rt, nk + 1), dtype), "dV": self.nan((rt, nv), dtype)}

        def launch(A, At, o, given):
            At.attention_bwd_kv(Kt, Vt, Qp, dOp, self.vec(given["lse"], H), self.vec(given["delta"], H), scale=scale, bias=bias, dK=o["dK"][:, :nk],
                                dV=o["dV"], heads=H)

        def check(o, what):
            assert np.isnan(o["dK"][:, nk:]).all(), (what, "padding written")
            got = {"dK": _named(o["dK"][:, :nk], snap.rm_t, what, "row that the row map does not name"),
                   "dV": _named(o["dV"], snap.rm_t, what, "row that the row map does not name")}
            self.finite(got, what)
            if bounded:
                for h, ref in enumerate(refs(True)):
                    _ratios("attention_bwd", dtype, BR.ratios({"dK": got["dK"][:, h * dk:(h + 1) * dk], "dV": got["dV"][:, h * dv:(h + 1) * dv]}, ref, dt), what)
        return Entry(make, launch, check, pre, bounded)

    # -- GAT and GATv2, with and without dropout
    def _gat(self, step, snap, v2):
        kind, _, dtype, bias, H, dv, drop, seed = step[:8]
        side = kind.split("_")[1] if "_" in kind else "fwd"
        use_pos = step[8] if side != "col" else False
        nv = H * dv
        dt = NP[dtype]
        pat, data = self.pat, self.data
        posd, posn = self.pos(use_pos)
        bounded = AP.bounded(step, self.model, self.prog.two_source)
        ra, rt = snap.rows_a, snap.rows_t
        dkw = dict(slope=AP.SLOPE, bias=bias, heads=H, dropout=drop, seed=seed)
        not_named = "row that the row map does not name"
        if v2:
            XT, dO = self.by_a("XT", data.XT[:, :nv], dtype, snap), self.by_a("XdO", data.XdO[:, :nv], dtype, snap)
            XS0, XS1 = self.sources("XS", data.XS[:, :nv], dtype)
            a_np = data.a_of(H, dv)
            a = self.plain("a", a_np, dtype)
            forward = lambda A, O, lse, p=None: A.gatv2_attention(XT, XS0, a, XS1=XS1, out=O, lse=self.vec(lse, H), p_out=None if p is None else self.vec(p, H),
                                                                  out_pos=posd if p is not None else None, **dkw)
        else:
            el, dO = self.by_a("el", data.el[:, :H], dtype, snap), self.by_a("GdO", data.GdO[:, :nv], dtype, snap)
            (er0, er1), (V0, V1) = self.sources("er", data.er[:, :H], dtype), self.sources("GV", data.GV[:, :nv], dtype)
            forward = lambda A, O, lse, p=None: A.gat_attention(el, er0, V0, er1=er1, V1=V1, out=O, lse=self.vec(lse, H),
                                                                p_out=None if p is None else self.vec(p, H), out_pos=posd if p is not None else None, **dkw)

        def ref(bwd):
            key = ("gref", v2, bwd, dtype, bias, H, dv, drop, seed if drop else None, snap.cur if bias else None, snap.map_a if drop else None)
            def make():
                val = snap.val if bias else None
                gdO = None if not bwd else (data.XdO if v2 else data.GdO)[:, :nv].astype(dt)
                kw = dict(rowmap=snap.rm_a, codes=pat.codes) if drop else {}
                if v2:
                    args = (pat.rp, pat.gcol, data.XT[:, :nv].astype(dt), data.XS[:, :nv].astype(dt), a_np.astype(dt), AP.SLOPE)
                    return DR.gatv2_reference(*args, drop, seed, val, gdO, **kw) if drop else G2.reference(*args, val, gdO)
                args = (pat.rp, pat.gcol, data.el[:, :H].astype(dt), data.er[:, :H].astype(dt), data.GV[:, :nv].astype(dt), AP.SLOPE)
                return DR.gat_reference(*args, drop, seed, val, gdO, **kw) if drop else G.reference(*args, val, gdO)
            return self.cached(key, make)

        tag = ("gatv2" if v2 else "gat") + (" dropout" if drop else "")
        if side == "fwd":
            make = lambda: {"O": self.nan((ra, nv + 3), dtype), "lse": self.nan((ra, H), dtype), "p": self.per_nnz(H, dtype, use_pos)}
            launch = lambda A, At, o, given: forward(A, o["O"][:, :nv], o["lse"], o["p"])

            def check(o, what):
                assert np.isnan(o["O"][:, nv:]).all(), (what, "padding written")
                got = {"O": _named(o["O"][:, :nv], snap.rm_a, what, not_named), "lse": _named(o["lse"], snap.rm_a, what, not_named),
                       "p": _named(o["p"], posn, what, "position that out_pos does not name")}
                self.finite(got, what, lse=("lse",))
                if bounded:
                    _ratios(tag, dtype, G.ratios(got, ref(False)), what)
            return Entry(make, launch, check, None, bounded)

        def pre(fA, fAt):
            O, lse = self.nan((ra, nv), dtype), self.nan((ra, H), dtype)
            forward(fA, O, lse)
            given = {"O": O, "lse": lse}
            if side == "col":
                delta = self.nan((ra, H), dtype)
                if v2:
                    fA.gatv2_attention_bwd_row(XT, XS0, a, O, dO, self.vec(lse, H), XS1=XS1, delta=self.vec(delta, H), **dkw)
                else:
                    fA.gat_attention_bwd_row(el, er0, V0, O, dO, self.vec(lse, H), er1=er1, V1=V1, delta=self.vec(delta, H), **dkw)
                given = {"lse": self.back(lse, snap), "delta": self.back(delta, snap)}
            return given

        if side == "row":
            wide = ("dXT", "da_part") if v2 else ()

            def make():
                o = {"delta": self.nan((ra, H), dtype), "ds": self.per_nnz(H, dtype, use_pos)}
                o.update({k: self.nan((ra, nv + 1), dtype) for k in wide} if v2 else {"d_el": self.nan((ra, H + 1), dtype)})
                return o

            def launch(A, At, o, given):
                common = dict(delta=self.vec(o["delta"], H), ds_out=self.vec(o["ds"], H), out_pos=posd, **dkw)
                if v2:
                    A.gatv2_attention_bwd_row(XT, XS0, a, given["O"], dO, self.vec(given["lse"], H), XS1=XS1, dXT=o["dXT"][:, :nv],
                                              da_part=o["da_part"][:, :nv], **common)
                else:
                    A.gat_attention_bwd_row(el, er0, V0, given["O"], dO, self.vec(given["lse"], H), er1=er1, V1=V1, d_el=o["d_el"][:, :H], **common)

            def check(o, what):
                got = {"delta": _named(o["delta"], snap.rm_a, what, not_named), "ds": _named(o["ds"], posn, what, "position that out_pos does not name")}
                for k, w in ((k, nv) for k in wide) if v2 else (("d_el", H),):
                    assert np.isnan(o[k][:, w:]).all(), (what, "padding written")
                    got[k] = _named(o[k][:, :w], snap.rm_a, what, not_named)
                self.finite(got, what)
                if bounded:
                    _ratios(tag, dtype, G.ratios(got, ref(True)), what)
            return Entry(make, launch, check, pre, bounded)

        # the column side on the single-source handle of A^T
        if v2:
            XSt, XTp, dOp = self.by_t("XS", data.XS[:, :nv], dtype, snap), self.plain("XT", data.XT[:, :nv], dtype), self.plain("XdO", data.XdO[:, :nv], dtype)
            make = lambda: {"dXS": self.nan((rt, nv + 2), dtype)}
            launch = lambda A, At, o, given: At.gatv2_attention_bwd_col(XSt, XTp, a, dOp, self.vec(given["lse"], H), self.vec(given["delta"], H),
                                                                        dXS=o["dXS"][:, :nv], **dkw)
            widths = {"dXS": nv}
        else:
            ert, Vt = self.by_t("er", data.er[:, :H], dtype, snap), self.by_t("GV", data.GV[:, :nv], dtype, snap)
            elp, dOp = self.plain("el", data.el[:, :H], dtype), self.plain("GdO", data.GdO[:, :nv], dtype)
            make = lambda: {"d_er": self.nan((rt, H + 1), dtype), "dV": self.nan((rt, nv + 2), dtype)}
            launch = lambda A, At, o, given: At.gat_attention_bwd_col(ert, Vt, elp, dOp, self.vec(given["lse"], H), self.vec(given["delta"], H),
                                                                      d_er=o["d_er"][:, :H], dV=o["dV"][:, :nv], **dkw)
            widths = {"d_er": H, "dV": nv}

        def check(o, what):
            got = {}
            for k, w in widths.items():
                assert np.isnan(o[k][:, w:]).all(), (what, "padding written")
                got[k] = _named(o[k][:, :w], snap.rm_t, what, not_named)
            self.finite(got, what)
            if bounded:
                _ratios(tag, dtype, G.ratios(got, ref(True)), what)
        return Entry(make, launch, check, pre, bounded)

    def _mask(self, step, snap):
        _, _, h, H, drop, seed, use_pos = step
        posd, posn = self.pos(use_pos)
        nnz = self.pat.gcol.size
        make = lambda: {"k": self.torch.full((nnz + (CP.OUT_EXTRA if use_pos else 0), H), FILL8, dtype=self.torch.uint8, device=self.gpu)}
        launch = lambda A, At, o, given: (A if h == "A" else At).dropout_mask(H, drop, seed, out=o["k"], out_pos=posd)
        want = AP.mask_of(self.data, h, snap.map_a if h == "A" else snap.map_t, H, drop, seed)

        def check(o, what):
            got = _named(o["k"], posn, what, "position that out_pos does not name")
            assert np.array_equal(got, want.astype(np.uint8)), (what, "the mask differs from numpy's Philox at %d entries" % int((got != want).sum()))
        return Entry(make, launch, check)

    def _product(self, step, snap, dtype, variant):
        from crp_spmm_amd import hip
        _, _, h, n = step
        pat, data, base = self.pat, self.data, self.data.base
        on_a = h == "A"
        src = base.B[:, :n] if on_a else base.Bt[:, :n]
        B0, B1 = self.sources("B", src, dtype) if on_a else (self.plain("Bt", src, dtype), None)
        rows, rm = (snap.rows_a, snap.rm_a) if on_a else (snap.rows_t, snap.rm_t)
        make = lambda: {"C": self.nan((rows, n + 2), dtype)}
        fn = hip.spmm_csr if dtype == "f64" else hip.spmm_csr_f32
        launch = lambda A, At, o, given: fn(A if on_a else At, B0, o["C"][:, :n], n=n, B1=B1, variant=variant)
        cur = data.sets[snap.cur]

        def check(o, what):
            assert np.isnan(o["C"][:, n:]).all(), (what, "padding written")
            got = _named(o["C"][:, :n], rm, what, "row that the row map does not name")
            if on_a:
                T1._check_product(dtype, cur.kind, pat.rp, pat.gcol, cur.val, src, None if cur.kind == "R" else base.product(cur, n), got, what)
            else:
                T1._check_product(dtype, cur.kind, pat.rpt, pat.cit, cur.val[pat.tmap], src, None if cur.kind == "R" else base.product_t(cur, n), got, what)
        return Entry(make, launch, check)

    def _spmm32(self, step, snap):
        return self._product(step, snap, "f32", 1)

    def _spmm64(self, step, snap):
        return self._product(step, snap, "f64", 1)

    def queries(self, A, At):
        return {"A.is_transposed": A.is_transposed, "T.is_transposed": At.is_transposed}

    def run(self, steps=None):
        """execute the program (or the given prefix), compare everything; returns the device time of the steps in ms"""
        torch, prog, model, data = self.torch, self.prog, self.model, self.data
        steps = list(prog.steps if steps is None else steps)
        final = [("spmm64", 0, "A", 7), ("spmm64", 1, "T", 7)]                     # the values are untouched
        plan = []
        for i, step in enumerate(steps + final):
            snap = self.snapshot()
            entry = self.build(step, snap) if step[0] not in AP.CTRL else None
            model.apply(step)
            plan.append((i, step, snap, entry, dict(model.queries())))
        # every call once on a fresh pair of handles made from what the model held: what a backward reads, and the bits to meet
        for i, step, snap, entry, _ in plan:
            if entry is None:
                continue
            try:
                fA, fAt = self.handles(snap)
                try:
                    entry.given = entry.pre(fA, fAt) if entry.pre is not None else None
                    entry.fresh = entry.make()
                    entry.launch(fA, fAt, entry.fresh, entry.given)
                    d = AP.dropout_of(step)
                    if d is not None and step[0] != "mask":
                        h = AP.handle_of(step)
                        got = (fA if h == "A" else fAt).dropout_mask(*d)
                        torch.cuda.synchronize()
                        want = AP.mask_of(data, h, snap.map_a if h == "A" else snap.map_t, *d)
                        assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8)), "the fresh pair's mask differs from numpy's Philox"
                    torch.cuda.synchronize()
                finally:
                    fA.free()
                    fAt.free()
            except Exception as e:
                raise AssertionError(self.report(i, step, steps, "on the fresh pair", e)) from e
        A, At = self.handles(Snap(data.sets[0].kind, data.sets[0].val, 0, 0, 0, data))
        lib = A._lib
        streams = Streams(lib, self.gpu)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(streams.s[0])
        streams.leave(0)
        try:
            for i, step, snap, entry, queries in plan:
                try:
                    s = streams.enter(step[1])
                    with torch.cuda.stream(s):
                        if step[0] == "update":
                            for H, src in ((A, step[2]), (At, step[3])):
                                H.update_values(data.sets[step[4]].val if src == "host" else self.vals_dev[step[4]], stream=s.cuda_stream)
                        elif step[0] == "rowmap":
                            A.set_rowmap(*((None, 0) if step[2] == 0 else data.rowmaps[step[2]]))
                        elif step[0] == "rowmapT":
                            At.set_rowmap(*((None, 0) if step[2] == 0 else data.rowmapsT[step[2]]))
                        else:
                            entry.launch(A, At, entry.outs, entry.given)
                    streams.leave(step[1])
                    assert self.queries(A, At) == queries, ("queries", self.queries(A, At), "the model says", queries)
                except Exception as e:
                    raise AssertionError(self.report(i, step, steps, "while issuing", e)) from e
            streams.s[0].wait_event(streams.last)
            t1.record(streams.s[0])
            torch.cuda.synchronize()                            # the ONE synchronisation
            ms = t0.elapsed_time(t1)
            host = lambda outs: {k: v.cpu().numpy() for k, v in outs.items()}
            for i, step, snap, entry, _ in plan:
                if entry is None:
                    continue
                try:
                    got = host(entry.outs)
                    what = (prog.seed, i, step)
                    entry.check(got, what)
                    _same_bits(got, host(entry.fresh), what)
                    if i < len(steps):
                        COUNTS["handle"][0] += 1
                        COUNTS["handle"][1] += 1
                        COUNTS["handle"][2] += bool(entry.bounded)
                except Exception as e:
                    raise AssertionError(self.report(i, step, steps, "wrong result", e)) from e
        finally:
            torch.cuda.synchronize()
            A.free()
            At.free()
            streams.close()
        return ms

    def report(self, i, step, steps, how, e):
        shown = self.prog._replace(steps=tuple(steps))
        if i >= len(steps):
            return "program seed %d (%s), %s at the closing variant-1 product %r after all %d steps: %s" % (
                self.prog.seed, self.prog.matrix, how, step, len(steps), e)
        return "program seed %d (%s), %s at step %d %r: %s\n%s" % (self.prog.seed, self.prog.matrix, how, i, step, e, AP.literal(shown, i))


def _clear_knobs(monkeypatch):
    for k in ("CRPSPMM_PANEL_ORDER", "CRPSPMM_TEAM2R", "CRPSPMM_REORDER"):
        monkeypatch.delenv(k, raising=False)


def _worst():
    return ", ".join("%s %.3g" % kv for kv in sorted(WORST.items()))


def _run_handle_program(gpu, monkeypatch, prog, steps=None):
    _clear_knobs(monkeypatch)
    t = time.perf_counter()
    ms = HandleRun(prog, gpu).run(steps)
    print("attention handle program %d (seed %d, %s%s): %d steps, %.1f ms on the device, %.2f s in all; steps / bitwise / bounded so far %r; "
          "worst error / bound so far: %s" % (prog.index, prog.seed, prog.matrix, ", two sources" if prog.two_source else "",
                                              len(prog.steps if steps is None else steps), ms, time.perf_counter() - t, COUNTS["handle"], _worst()))


@pytest.mark.parametrize("index", range(AP.HANDLE_PROGRAMS))
def test_handle_program(crp, gpu, monkeypatch, index):
    _run_handle_program(gpu, monkeypatch, AP.handle_programs()[index])


# ---- the row engine ----------------------------------------------------------------------------------------------------------------

class EngineRun(T1.Base):
    """RpSpmm over the given communicator, on this rank's rows [s0, e0) of A and rows [b0, b1) of B (B's displacements: bd)"""

    def __init__(self, prog, n, gpu, comm, rows, bd, several):
        self.prog, self.n, self.comm, self.several = prog, n, comm, several
        pat, data, self.model = AP.engine_setup(prog, n)
        super().__init__(gpu, data)
        self.s0, self.e0 = int(rows[0]), int(rows[1])
        self.bd = np.asarray(bd, np.int32)
        self.b0, self.b1 = int(self.bd[comm.rank]), int(self.bd[comm.rank + 1])
        self.lo, self.hi = int(pat.rp[self.s0]), int(pat.rp[self.e0])
        self.m, self.kb, self.nnz = self.e0 - self.s0, self.b1 - self.b0, self.hi - self.lo
        self.rp_loc = (pat.rp[self.s0:self.e0 + 1] - pat.rp[self.s0]).astype(np.int32)
        self.rpt_loc = (pat.rpt[self.b0:self.b1 + 1] - pat.rpt[self.b0]).astype(np.int32)
        self.tlo, self.thi = int(pat.rpt[self.b0]), int(pat.rpt[self.b1])
        self.vals_dev = {"f64": [self.dev(vs.val[self.lo:self.hi]) for vs in data.sets],
                         "f32": [self.dev(vs.val[self.lo:self.hi].astype(np.float32)) for vs in data.sets]}

    def engine(self):
        from crp_spmm_amd import engine
        pat = self.pat
        val = self.data.sets[0].val
        return engine.RpSpmm(self.s0, self.m, pat.rp[self.s0:self.e0 + 1], pat.gcol[self.lo:self.hi], val[self.lo:self.hi], self.bd, self.n, self.comm)

    def snapshot(self):
        m = self.model
        s = Snap(m.kind(), m.current_values(), m.cur, 0, 0, self.data)
        s.set = self.data.sets[m.cur]
        return s

    def block(self, name, a, r0, r1, dtype, where, layout):
        """rows [r0, r1) of a dense operand as the engine takes it: layout 1 as an (n, rows) array holding the column-major data"""
        def make():
            x = a[r0:r1].astype(NP[dtype])
            x = np.array(x.T if layout else x, order="C")
            return self.dev(x) if where == "dev" else x
        return self.cached((name, dtype, where, layout, a.shape), make)

    def full(self, name, a, dtype):
        return self.cached((name + "/full", dtype, a.shape), lambda: self.dev(np.ascontiguousarray(a).astype(NP[dtype])))

    def result(self, rows, dtype, where, layout, n=None):
        n = self.n if n is None else n
        if where == "host":
            return np.full((n, rows) if layout else (rows, n), np.nan, NP[dtype])
        return self.nan((n, rows + 3) if layout else (rows, n + 3), dtype)

    def view(self, C, rows, where, layout):
        return C if where == "host" else (C[:, :rows] if layout else C[:, :self.n])

    def vector(self, shape, dtype, where):
        return np.full(shape, np.nan, NP[dtype]) if where == "host" else self.nan(shape, dtype)

    @staticmethod
    def flat(t, H):
        return t.reshape(-1) if H == 1 else t

    def body(self, got, rows, layout, what):
        n = self.n
        if layout:
            assert np.isnan(got[:, rows:]).all(), (what, "padding written")
            return np.ascontiguousarray(got[:, :rows].T)
        assert np.isnan(got[:, n:]).all(), (what, "padding written")
        return np.ascontiguousarray(got[:, :n])

    def build(self, step, snap):
        return getattr(self, "_" + step[0])(step, snap)

    def _product(self, step, snap, transposed):
        _, _, dtype, where, layout = step
        pat, base, n = self.pat, self.data.base, self.n
        cur = snap.set
        want = None if cur.kind == "R" else (base.product_t(cur, n) if transposed else base.product(cur, n))
        if transposed:
            src, rows, B = base.Bt[:, :n], self.kb, self.block("Bt", base.Bt[:, :n], self.s0, self.e0, dtype, where, layout)
            sub = (self.rpt_loc, pat.cit[self.tlo:self.thi], snap.val[pat.tmap][self.tlo:self.thi], self.b0, self.b1)
        else:
            src, rows, B = base.B[:, :n], self.m, self.block("B", base.B[:, :n], self.b0, self.b1, dtype, where, layout)
            sub = (self.rp_loc, pat.gcol[self.lo:self.hi], snap.val[self.lo:self.hi], self.s0, self.e0)
        make = lambda: {"C": self.result(rows, dtype, where, layout)}

        def launch(e, outs, stream):
            view = self.view(outs["C"], rows, where, layout)
            if transposed:
                (e.exec_t if dtype == "f64" else e.exec_t_f32)(layout, B, view, stream=stream)
            else:
                e.exec(layout, B, view, stream=stream)

        def check(outs, what):
            got = self.body(outs["C"], rows, layout, what)
            if rows:
                T1._check_product(dtype, snap.kind, sub[0], sub[1], sub[2], src, None if want is None else want[sub[3]:sub[4]], got, what)
        return Entry(make, launch, check, None, not CP.exact_in(snap.kind, dtype))

    def _exec(self, step, snap):
        return self._product(step, snap, False)

    def _exec_t(self, step, snap):
        return self._product(step, snap, True)

    def _sddmm(self, step, snap):
        _, _, dtype, mode, where = step
        pat, base, n = self.pat, self.data.base, self.n
        X, Y = self.block("X", base.X[:, :n], self.s0, self.e0, dtype, where, 0), self.block("Y", base.Y[:, :n], self.b0, self.b1, dtype, where, 0)
        cur = snap.set
        want = base.sddmm(cur, mode, n) if (mode == 0 or cur.kind != "R") else None
        make = lambda: {"out": self.vector((self.nnz,), dtype, where)}
        launch = lambda e, outs, stream: e.sddmm(0, X, Y, outs["out"], mode=mode, stream=stream)
        lo, hi = self.lo, self.hi

        def check(outs, what):
            got = outs["out"]
            assert got.dtype == NP[dtype] and got.shape == (self.nnz,), (what, got.dtype, got.shape)
            if mode == 0 or CP.exact_in(snap.kind, dtype):
                w = want[lo:hi].astype(NP[dtype])
                assert np.array_equal(got, w), (what, "differs from the exact dots at %d entries" % int((got != w).sum()))
                return
            X_, Y_ = base.X[:, :n].astype(np.longdouble), base.Y[:, :n].astype(np.longdouble)
            prod = X_[pat.rows[lo:hi]] * Y_[pat.gcol[lo:hi]]
            a = snap.val[lo:hi].astype(np.longdouble)
            ref, S = a * prod.sum(axis=1), np.abs(prod).sum(axis=1)
            bound = (n + (2 if dtype == "f64" else 3)) * T1.U[dtype] * np.abs(a) * S          # tests/test_gpu_sddmm.py
            assert np.isfinite(got).all(), (what, "non-finite output")
            w = SR.worst(got, ref, bound)[0] if got.size else 0.0
            _note("sddmm mode 1 " + dtype, w)
            assert w <= 1, (what, "dot bound missed", w)
        return Entry(make, launch, check, None, not (mode == 0 or CP.exact_in(snap.kind, dtype)))

    def _softmax(self, step, snap, bwd=False):
        dtype = step[2]
        dt = NP[dtype]
        data, pat = self.data.base, self.pat
        ref = self.cached(("sref", dtype), lambda: SR.reference_fwd(pat.rp, data.scores.astype(dt)))[0]
        y_full, s_full, dy_full = self.full("y", ref.astype(dt), dtype), self.full("s", data.scores, dtype), self.full("dy", data.grads, dtype)
        lo, hi = self.lo, self.hi
        make = lambda: {"out": self.nan((self.nnz,), dtype)}

        def launch(e, outs, stream):
            if bwd:
                e.row_softmax_bwd(y_full[lo:hi], dy_full[lo:hi], out=outs["out"], stream=stream)
            else:
                e.row_softmax(s_full[lo:hi], out=outs["out"], stream=stream)

        def oracle(A, At):
            out = self.nan((pat.gcol.size,), dtype)
            if bwd:
                A.row_softmax_bwd(y_full, dy_full, out=out)
            else:
                A.row_softmax(s_full, out=out)
            return {"out": out[lo:hi]}

        def check(outs, what):
            assert np.isfinite(outs["out"]).all(), (what, "non-finite output")
        e = Entry(make, launch, check)
        e.oracle = oracle
        return e

    def _softmax_bwd(self, step, snap):
        return self._softmax(step, snap, True)

    def _fused(self, step, snap, kind):
        """attn / gat / gatv2: (kind, s, dtype, bias, H, where[, layout])"""
        dtype, bias, H, where = step[2:6]
        layout = step[6] if kind != "attn" else 0
        pat, data, n = self.pat, self.data, self.n
        s0, e0, b0, b1, lo, hi = self.s0, self.e0, self.b0, self.b1, self.lo, self.hi
        scale = 1.0 / np.sqrt(n // H)
        if kind == "attn":
            Qb, Kb, Vb = (self.block(k, getattr(data, k)[:, :n], r0, r1, dtype, where, 0) for k, r0, r1 in (("Q", s0, e0), ("K", b0, b1), ("V", b0, b1)))
            Qf, Kf, Vf = (self.full(k, getattr(data, k)[:, :n], dtype) for k in "QKV")
        elif kind == "gat":
            elf, erf, Vf = self.full("el", data.el[:, :H], dtype), self.full("er", data.er[:, :H], dtype), self.full("GV", data.GV[:, :n], dtype)
            Vb = self.block("GV", data.GV[:, :n], b0, b1, dtype, where, layout)
        else:
            XTf, XSf = self.full("XT", data.XT[:, :n], dtype), self.full("XS", data.XS[:, :n], dtype)
            af = self.full("a%d" % H, data.a_of(H, n // H), dtype)
            XSb = self.block("XS", data.XS[:, :n], b0, b1, dtype, where, layout)
        make = lambda: {"O": self.result(self.m, dtype, where, layout), "lse": self.vector((self.m, H), dtype, where),
                        "p": self.vector((self.nnz, H), dtype, where)}

        def launch(e, outs, stream):
            O = self.view(outs["O"], self.m, where, layout)
            kw = dict(bias=bias, lse=self.flat(outs["lse"], H), p_out=self.flat(outs["p"], H), stream=stream, heads=H)
            if kind == "attn":
                e.attention(0, Qb, Kb, Vb, O, scale=scale, **kw)
            elif kind == "gat":
                e.gat_attention(layout, elf[s0:e0], erf[b0:b1], Vb, O, slope=AP.SLOPE, **kw)
            else:
                e.gatv2_attention(layout, XTf[s0:e0], af, XSb, O, slope=AP.SLOPE, **kw)

        def oracle(A, At):
            full = pat.m
            O, lse, p = self.nan((full, n), dtype), self.nan((full, H), dtype), self.nan((pat.gcol.size, H), dtype)
            kw = dict(bias=bias, out=O, lse=self.flat(lse, H), p_out=self.flat(p, H), heads=H)
            if kind == "attn":
                A.attention(Qf, Kf, Vf, scale=scale, **kw)
            elif kind == "gat":
                A.gat_attention(elf, erf, Vf, slope=AP.SLOPE, **kw)
            else:
                A.gatv2_attention(XTf, XSf, af, slope=AP.SLOPE, **kw)
            return {"O": O[s0:e0], "lse": lse[s0:e0], "p": p[lo:hi]}

        live = np.diff(self.rp_loc) > 0

        def check(outs, what):
            outs["O"] = self.body(outs["O"], self.m, layout, what)
            assert np.isfinite(outs["O"]).all() and np.isfinite(outs["p"]).all(), (what, "non-finite output")
            assert np.isfinite(outs["lse"][live]).all() and (outs["lse"][~live] == -np.inf).all(), (what, "lse of empty rows")
        e = Entry(make, launch, check)
        e.oracle = oracle
        return e

    def _attn(self, step, snap):
        return self._fused(step, snap, "attn")

    def _gat(self, step, snap):
        return self._fused(step, snap, "gat")

    def _gatv2(self, step, snap):
        return self._fused(step, snap, "gatv2")

    def _attn_bwd(self, step, snap):
        _, _, dtype, bias, H = step
        pat, data, n = self.pat, self.data, self.n
        dt = NP[dtype]
        s0, e0, b0, b1, lo, hi = self.s0, self.e0, self.b0, self.b1, self.lo, self.hi
        d = n // H
        scale = 1.0 / np.sqrt(d)
        Qf, Kf, Vf, dOf = (self.full(k, getattr(data, k)[:, :n], dtype) for k in ("Q", "K", "V", "dO"))
        m, kb, nnz = self.m, self.kb, self.nnz
        make = lambda: {"O": self.nan((m, n), dtype), "lse": self.nan((m, H), dtype), "dQ": self.nan((m, n + 1), dtype),
                        "dK": self.nan((kb, n + 2), dtype), "dV": self.nan((kb, n), dtype), "ds": self.nan((nnz, H), dtype)}

        def launch(e, outs, stream):
            e.attention(0, Qf[s0:e0], Kf[b0:b1], Vf[b0:b1], outs["O"], scale=scale, bias=bias, lse=self.flat(outs["lse"], H), stream=stream, heads=H)
            e.attention_bwd(Qf[s0:e0], Kf[b0:b1], Vf[b0:b1], outs["O"], dOf[s0:e0], self.flat(outs["lse"], H), outs["dQ"][:, :n], outs["dK"][:, :n],
                            outs["dV"], scale=scale, bias=bias, ds_out=self.flat(outs["ds"], H), stream=stream, heads=H)

        def oracle(A, At):
            full, k = pat.m, pat.k
            O, lse, delta = self.nan((full, n), dtype), self.nan((full, H), dtype), self.nan((full, H), dtype)
            dQ, dK, dV, ds = self.nan((full, n), dtype), self.nan((k, n), dtype), self.nan((k, n), dtype), self.nan((pat.gcol.size, H), dtype)
            A.attention(Qf, Kf, Vf, scale=scale, bias=bias, out=O, lse=self.flat(lse, H), heads=H)
            A.attention_bwd_q(Qf, Kf, Vf, O, dOf, self.flat(lse, H), scale=scale, bias=bias, dQ=dQ, delta=self.flat(delta, H), ds_out=self.flat(ds, H), heads=H)
            At.attention_bwd_kv(Kf, Vf, Qf, dOf, self.flat(lse, H), self.flat(delta, H), scale=scale, bias=bias, dK=dK, dV=dV, heads=H)
            out = {"O": O[s0:e0], "lse": lse[s0:e0], "dQ": dQ[s0:e0], "ds": ds[lo:hi]}
            if not self.several:
                out.update({"dK": dK[b0:b1], "dV": dV[b0:b1]})
            return out

        def check(outs, what):
            for k_, w in (("dQ", n), ("dK", n)):
                assert np.isnan(outs[k_][:, w:]).all(), (what, "padding written")
                outs[k_] = np.ascontiguousarray(outs[k_][:, :w])
            for k_ in ("dQ", "dK", "dV", "ds", "O"):
                assert np.isfinite(outs[k_]).all(), (what, k_, "non-finite output")
            if self.several and kb:
                assert (not bias) or snap.kind == "R", (what, "the generator draws a bias at several ranks under the R set only")
                for h in range(H):
                    sl = slice(h * d, (h + 1) * d)
                    ref = self.cached(("bref", dtype, bias, H, h, snap.cur if bias else None), lambda: BR.reference(
                        pat.rp, pat.gcol, data.Q[:, :n][:, sl].astype(dt), data.K[:, :n][:, sl].astype(dt), data.V[:, :n][:, sl].astype(dt),
                        data.dO[:, :n][:, sl].astype(dt), dt(scale), snap.val.astype(dt) if bias else None, ncol=pat.k))
                    for k_, bound in (("dK", BR.bound_dK), ("dV", BR.bound_dV)):
                        w = BR.worst(outs[k_][:, sl].ravel(), ref[k_][b0:b1].ravel(), np.asarray(bound(ref, dt))[b0:b1].ravel())[0]
                        _note("attention_bwd %s %s, several ranks" % (k_, dtype), w)
                        assert w <= 1, (what, "backward bound missed", k_, h, w)
        e = Entry(make, launch, check, None, self.several)
        e.oracle = oracle
        return e

    def queries(self, e):
        return {"transposed_built": e.transposed_built, "sddmm_built": e.sddmm_built, "attention_built": e.attention_built(),
                "attention_bwd_built": e.attention_bwd_built(), "row_softmax_built": e.row_softmax_built,
                "host_values_stale": e.host_values_stale, "gat_built": e.gat_built(), "gatv2_built": e.gatv2_built()}

    def run(self, steps=None):
        from crp_spmm_amd import hip
        torch, prog, model, pat, data = self.torch, self.prog, self.model, self.pat, self.data
        steps = list(prog.steps if steps is None else steps)
        final = [("set_variant", 0, 1), ("exec", 1, "f64", "dev", 0)]                   # the values are untouched
        control = ("update", "update_dev", "set_variant", "set_variant_f32", "set_timing")
        plan = []
        for i, step in enumerate(steps + final):
            snap = self.snapshot()
            entry = self.build(step, snap) if step[0] not in control else None
            model.apply(step)
            plan.append((i, step, snap, entry, dict(model.queries())))
        e = self.engine()
        streams = Streams(e._lib, self.gpu)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(streams.s[0])
        streams.leave(0)
        lo, hi = self.lo, self.hi
        wrong = None
        try:
            for i, step, snap, entry, queries in plan:
                try:
                    s = streams.enter(step[1])
                    with torch.cuda.stream(s):
                        if step[0] == "update":
                            e.update_values(data.sets[step[2]].val[lo:hi])
                        elif step[0] == "update_dev":
                            e.update_values_dev(self.vals_dev[step[3]][step[2]], stream=s.cuda_stream)
                        elif step[0] == "set_variant":
                            e.set_variant(step[2])
                        elif step[0] == "set_variant_f32":
                            e.set_variant_f32(step[2])
                        elif step[0] == "set_timing":
                            e.set_timing(step[2])
                        else:
                            entry.launch(e, entry.outs, s.cuda_stream)
                    streams.leave(step[1])
                    got = self.queries(e)
                    # (a rank without nonzeros has no host values to fall behind: crp_rp_spmm_update_values_dev returns at once)
                    queries["host_values_stale"] = queries["host_values_stale"] and self.nnz > 0
                    if got != queries and wrong is None:
                        # held back until every step is issued: the steps are collective, and a rank that stopped here would leave
                        # its peers inside an exchange
                        wrong = AssertionError(self.report(i, step, steps, "while issuing", ("queries", got, "the model says", queries)))
                except Exception as ex:
                    raise Stranded(self.report(i, step, steps, "while issuing", ex)) from ex
            streams.s[0].wait_event(streams.last)
            t1.record(streams.s[0])
            torch.cuda.synchronize()                            # the ONE synchronisation
            ms = t0.elapsed_time(t1)
            if wrong is not None:
                raise wrong
            host = lambda outs: {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in outs.items()}
            for i, step, snap, entry, _ in plan:
                if entry is None:
                    continue
                try:
                    what = (prog.seed, self.comm.rank, i, step)
                    got = host(entry.outs)
                    entry.check(got, what)
                    oracle = getattr(entry, "oracle", None)
                    if oracle is not None:
                        # this rank's slice of the handle calls on a fresh pair of handles of the full matrix at the model's values
                        fA = hip.CsrDev(pat.m, pat.k, pat.rp, pat.gcol, snap.val)
                        fAt = hip.CsrDev.from_transpose(pat.m, pat.k, pat.rp, pat.gcol, snap.val) if step[0] == "attn_bwd" else None
                        try:
                            fresh = oracle(fA, fAt)
                            torch.cuda.synchronize()
                            _same_bits(got, host(fresh), what)
                        finally:
                            fA.free()
                            if fAt is not None:
                                fAt.free()
                    if i < len(steps):
                        COUNTS["engine"][0] += 1
                        COUNTS["engine"][1] += oracle is not None or not entry.bounded
                        COUNTS["engine"][2] += bool(entry.bounded)
                except Exception as ex:
                    raise AssertionError(self.report(i, step, steps, "wrong result", ex)) from ex
        finally:
            torch.cuda.synchronize()
            e.free()
            streams.close()
        return ms

    def report(self, i, step, steps, how, e):
        shown = self.prog._replace(steps=tuple(steps))
        head = "engine program seed %d (%s, glb_n %d, rank %d of %d, rows %d:%d, B rows %d:%d)" % (
            self.prog.seed, self.prog.matrix, self.n, self.comm.rank, self.comm.nproc, self.s0, self.e0, self.b0, self.b1)
        if i >= len(steps):
            return "%s, %s at the closing variant-1 product %r after all %d steps: %s" % (head, how, step, len(steps), e)
        return "%s, %s at step %d %r: %s\n%s" % (head, how, i, step, e, AP.literal(shown, i))


@pytest.mark.parametrize("index", range(AP.ENGINE_PROGRAMS))
def test_rp_engine_program(crp, gpu, monkeypatch, index):
    from crp_spmm_amd import comm
    _clear_knobs(monkeypatch)
    prog, n = AP.engine_programs(False)[index]
    pat = AP.pattern(prog.matrix, False)
    sc = comm.SelfComm()
    t = time.perf_counter()
    try:
        ms = EngineRun(prog, n, gpu, sc, (0, pat.m), [0, pat.k], False).run()
    finally:
        sc.free()
    print("attention engine program %d (seed %d, %s, glb_n %d): %d steps, %.1f ms on the device, %.2f s in all; steps / bitwise / bounded so far %r; "
          "worst error / bound so far: %s" % (index, prog.seed, prog.matrix, n, len(prog.steps), ms, time.perf_counter() - t, COUNTS["engine"], _worst()))


def test_an_engine_without_rows_takes_empty_host_operands(crp, gpu, monkeypatch):
    """The prefix at which the several-rank program on the layout with a rank without rows of A first failed: a GATv2 step with
    column-major operands on the host.  That rank's O is an (n, 0) numpy array, to which numpy gives strides of 0, and the engine's
    wrappers refused it before the library was called.  Here on one rank without rows, over SelfComm."""
    from crp_spmm_amd import comm
    _clear_knobs(monkeypatch)
    prog, n = AP.engine_programs(True)[2]
    steps = prog.steps[:3]
    assert steps[2][0] == "gatv2" and steps[2][5:] == ("host", 1)
    pat = AP.pattern(prog.matrix, False)
    sc = comm.SelfComm()
    try:
        EngineRun(prog, n, gpu, sc, (0, 0), [0, pat.k], False).run(steps)
    finally:
        sc.free()


@pytest.mark.parametrize("world", [2, 4])
def test_rp_engine_programs_on_several_ranks(world):
    """tests/gpu_dist_attention_programs_worker.py: the several-rank family on `world` ranks that share one GPU, device payloads
    staged through the host"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    for k in ("CRPSPMM_EXPECT_NATIVE_RCCL", "CRPSPMM_PANEL_ORDER", "CRPSPMM_TEAM2R", "CRPSPMM_REORDER"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(30420 + world), os.path.join(ROOT, "tests", "gpu_dist_attention_programs_worker.py")]
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-6000:]
    assert "GPU_DIST_ATTENTION_PROGRAMS_WORKER_OK world=%d" % world in r.stdout
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("attention engine program")))
    print("world %d: %.2f s in all" % (world, time.perf_counter() - t))
