"""GPU: one handle pair and one engine run through the seeded programs of tests/call_programs.py, every step checked against
the model.

The runner executes a program step by step.  Every output goes into its own NaN-filled device tensor, allocated with its
padding before the first step.  The steps alternate between the default stream and two non-blocking streams, as the program
says; consecutive steps are ordered by an event only (record behind the step, wait_event before the next) and the host never
waits between them: "state a call builds on a handle is complete on return" (include/crpspmm_hip.h) is what makes that
legal.  After ONE synchronisation at the end every output is compared:

    products, transposed products, SDDMM     bit for bit under an E32 set (both dtypes) and under an E64 set in fp64;
                                             check_f64_bound / check_f32_bound and the SDDMM's per-entry dot bound otherwise
    attention, its backward, the softmax     bit for bit against the same call on a FRESH pair of handles made from the model's
                                             current values (the bits depend on the row's entries in CSR order only: DESIGN 5j,
                                             5l), finite, and -- wherever the values do not enter or are an R set -- inside the
                                             derived bounds of attention_ref / attention_bwd_ref / softmax_ref
    around every output                      padding columns, rows of C the row map does not name and positions out_pos does
                                             not name still hold NaN
    after every step                         the queries equal the model's (a value update builds nothing)
    after the last step                      a variant-1 product equals the model's: the values are untouched

A failure names the program's seed, the step's index and the step, and prints the prefix up to it as a literal.

Engines: RpSpmm and Para2dSpmm (1 x 1) over comm.SelfComm, in this process.  Their fused attention, its backward and the softmax
are compared with the device handle calls on fresh handles (include/crp_engine.h: at one rank the engine's results equal them).
Engines of several ranks -- split into interior and boundary rows, with sums that cross ranks, or on a grid -- are not run through
programs here; tests/gpu_dist_*_worker.py cover them call by call.

The handle's own processing order of the rows (crp_csr_dev::ord with f_val and rowmap_fmt) exists only for square single-source
matrices of at least 2048 rows (csrc/dispatch.cpp, format_order): the eight programs, of a few hundred rows, never meet it -- what
two of them run under CRPSPMM_PANEL_ORDER=1 is the row panels' processing order.  A ninth program on 2048 rows under
CRPSPMM_REORDER=1 does.

Each test prints the device time of its steps, its wall time and the worst error-to-bound ratios seen so far.
"""
import ctypes as C
import time

import numpy as np
import pytest

import attention_bwd_ref as BR
import attention_ref as R
import call_programs as CP
import fp32_ref
import fp64_ref
import softmax_ref as SR

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
WORST = {}                          # operation -> worst |got - ref| / bound seen in this process
A_WAS_REORDERED = []                # crp_csr_dev_reordered of the handle pair of every handle run, in order


def _note(op, ratio):
    WORST[op] = max(WORST.get(op, 0.0), float(ratio))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


class Streams:
    """the default stream and two non-blocking ones (crp_stream_create: hipStreamNonBlocking), and the event chain"""

    def __init__(self, lib, gpu):
        import torch
        self.lib, self.raw = lib, []
        self.s = [torch.cuda.default_stream(gpu)]
        for _ in range(2):
            p = C.c_void_p()
            assert lib.crp_stream_create(C.byref(p)) == 0
            self.raw.append(p)
            self.s.append(torch.cuda.ExternalStream(p.value, device=gpu))
        self.last = None

    def enter(self, i):
        """the stream of the next step, made to wait for the step before it"""
        if self.last is not None:
            self.s[i].wait_event(self.last)
        return self.s[i]

    def leave(self, i):
        import torch
        self.last = torch.cuda.Event()
        self.last.record(self.s[i])

    def close(self):
        for p in self.raw:
            self.lib.crp_stream_destroy(p)


def _ratio_f64(rp, ci, val, B, Cgot, what):
    return fp64_ref.check_f64_bound(rp, ci, val, B, Cgot, what)


def _ratio_f32(rp, ci, val, B32, Cgot, what):
    rb = fp32_ref.f32_bound(rp, ci, val, B32)
    fp32_ref.check_f32_bound(rp, ci, val, B32, Cgot, what, ref_bound=rb)
    err = np.abs(np.asarray(Cgot, dtype=np.float64) - rb[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / rb[1])
    return float(ratio.max()) if ratio.size else 0.0


def _check_product(dtype, kind, rp, ci, val, B, want, got, what):
    """got: the named rows of C in the dtype; want: the model's exact product or None"""
    assert got.dtype == NP[dtype] and got.shape == (rp.size - 1, B.shape[1]), (what, got.dtype, got.shape)
    if CP.exact_in(kind, dtype):
        assert np.array_equal(got, want.astype(NP[dtype])), (what, "differs from the exact product at %d entries" % int((got != want.astype(NP[dtype])).sum()),
                                                             np.argwhere(got != want.astype(NP[dtype]))[:4].tolist())
    elif dtype == "f64":
        _note("product f64", _ratio_f64(rp, ci, val, B, got, what))
    else:
        _note("product f32", _ratio_f32(rp, ci, val, B.astype(np.float32), got, what))


def _check_sddmm(dtype, kind, mode, data, vs_val, want, n, got, what):
    pat = data.pat
    assert got.dtype == NP[dtype] and got.shape == (pat.gcol.size,), (what, got.dtype, got.shape)
    if mode == 0 or CP.exact_in(kind, dtype):
        want = want.astype(NP[dtype])
        assert np.array_equal(got, want), (what, "differs from the exact dots at %d entries" % int((got != want).sum()))
        return
    X, Y = data.X[:, :n].astype(np.longdouble), data.Y[:, :n].astype(np.longdouble)       # (exact in fp32 as well)
    prod = X[pat.rows] * Y[pat.gcol]
    a = vs_val.astype(np.longdouble)
    ref, S = a * prod.sum(axis=1), np.abs(prod).sum(axis=1)
    bound = (n + (2 if dtype == "f64" else 3)) * U[dtype] * np.abs(a) * S          # tests/test_gpu_sddmm.py
    assert np.isfinite(got).all(), (what, "non-finite output")
    w, at = SR.worst(got, ref, bound)
    _note("sddmm mode 1 " + dtype, w)
    assert w <= 1, (what, "dot bound missed", w, at)


def _check_attention(dtype, ref, O, lse, p, what):
    assert np.isfinite(O).all() and np.isfinite(p).all(), (what, "non-finite output")
    live = np.isfinite(ref["lse"].astype(np.float64))
    assert np.array_equal(np.isfinite(lse), live) and (lse[~live] == -np.inf).all(), (what, "lse of empty rows")
    if ref.get("bounded"):
        dt = NP[dtype]
        wo = R.worst(O.ravel(), ref["O"].ravel(), R.bound_O(ref, dt).ravel())[0]
        wp = R.worst(p, ref["p"], R.bound_p(ref, dt))[0]
        wl = R.worst(lse[live], ref["lse"][live], R.bound_lse(ref, dt)[live])[0]
        for k, w in (("O", wo), ("p_out", wp), ("lse", wl)):
            _note("attention %s %s" % (k, dtype), w)
        assert wo <= 1 and wp <= 1 and wl <= 1, (what, "attention bound missed", wo, wp, wl)


def _same_bits(got, fresh, what):
    for name in got:
        assert np.array_equal(_bits(got[name]), _bits(fresh[name])), \
            (what, "%s differs from the same call on fresh handles at %d entries" % (name, int((_bits(got[name]) != _bits(fresh[name])).sum())))


class Snapshot:
    """what the model held when a step was issued"""

    def __init__(self, kind, val, rowmap, c_nrow):
        self.kind, self.val, self.rowmap, self.c_nrow = kind, val, rowmap, c_nrow


class Base:
    def __init__(self, gpu, data):
        import torch
        self.torch, self.gpu, self.data, self.pat = torch, gpu, data, data.pat
        self.TD = {"f64": torch.float64, "f32": torch.float32}
        self._cache = {}

    def dev(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).to(self.gpu)          # (a copy: the data arrays are read-only)

    def nan(self, shape, dtype):
        return self.torch.full(tuple(shape), float("nan"), dtype=self.TD[dtype], device=self.gpu)

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def padded(self, a, dtype, pad):
        """(the tensor that owns the memory, the view of a's shape)"""
        t = self.torch.zeros((a.shape[0], a.shape[1] + pad), dtype=self.TD[dtype], device=self.gpu)
        t[:, :a.shape[1]] = self.dev(a.astype(NP[dtype]))
        return t[:, :a.shape[1]] if pad else t

    def mapped(self, a, dtype, snap):
        """a's rows at the rows the row map names of a NaN-filled array of c_nrow rows"""
        if snap.rowmap is None:
            return self.dev(a.astype(NP[dtype]))
        full = np.full((snap.c_nrow,) + a.shape[1:], np.nan, NP[dtype])
        full[snap.rowmap] = a
        return self.dev(full)

    def split(self, a, dtype, pad=0):
        """(first source, second source or None) of an operand with a row per column of A"""
        pat = self.pat
        if not pat.remote.size:
            return self.padded(a, dtype, pad), None
        return self.padded(a[pat.lo:pat.hi], dtype, pad), self.padded(a[pat.remote], dtype, pad)

    @staticmethod
    def named_rows(body, snap, what):
        """the rows of an output that the row map names; every other row must still hold NaN"""
        if snap.rowmap is None:
            return body
        rest = np.ones(body.shape[0], bool)
        rest[snap.rowmap] = False
        assert np.isnan(body[rest]).all(), (what, "a row that the row map does not name was written")
        return body[snap.rowmap]

    @staticmethod
    def named_pos(out, pos, what):
        if pos is None:
            return out
        rest = np.ones(out.size, bool)
        rest[pos] = False
        assert np.isnan(out[rest]).all(), (what, "a position that out_pos does not name was written")
        return out[pos]

    def attention_ref(self, dtype, bias, nk, nv, snap, val):
        """attention_ref.reference on the dtype-rounded operands; "bounded": the derived bounds apply (the values do not enter, or
        they are an R set: under an E set the bias is steep beyond the bounds' data rule)"""
        dt = NP[dtype]
        d = self.data
        key = ("aref", dtype, bias, nk, nv, id(val) if bias else None)
        def make():
            ref = R.reference(self.pat.rp, self.pat.gcol, d.Q[:, :nk].astype(dt), d.K[:, :nk].astype(dt), d.V[:, :nv].astype(dt),
                              dt(1.0 / np.sqrt(nk)), val.astype(dt) if bias else None)
            ref["bounded"] = (not bias) or snap.kind == "R"
            return ref
        return self.cached(key, make)


# ---- the device handles ----------------------------------------------------------------------------------------------------------

class HandleRun(Base):
    def __init__(self, prog, gpu):
        self.prog = prog
        pat, data, self.model = CP.handle_setup(prog)
        super().__init__(gpu, data)
        self.vals_dev = [self.dev(vs.val) for vs in data.sets]
        self.pos_dev = self.dev(data.out_pos)
        self.pos_np = data.out_pos.astype(np.int64)

    def handles(self, val, snap):
        from crp_spmm_amd import hip
        pat = self.pat
        A = hip.CsrDev(pat.m, pat.ncol0, pat.rp, pat.codes, val)
        At = hip.CsrDev.from_transpose(pat.m, pat.k, pat.rp, pat.gcol, val)
        if snap is not None and snap.rowmap is not None:
            A.set_rowmap(snap.rowmap, snap.c_nrow)
        return A, At

    def snapshot(self):
        rm, c_nrow = self.model.rowmap()
        return Snapshot(self.model.values.kind, self.model.values.val, rm, c_nrow)

    # every builder returns (outputs: name -> tensor factory result, launch(A, At, outs), check(outs as numpy), replay?)
    def build(self, step, snap):
        return getattr(self, "_" + step[0])(step, snap)

    def _spmm(self, step, snap):
        from crp_spmm_amd import hip
        _, _, dtype, h, variant, n, layout, pad = step
        pat, data = self.pat, self.data
        on_a = h == "A"
        src = data.B[:, :n] if on_a else data.Bt[:, :n]
        rows_out = snap.c_nrow if on_a else pat.k
        if layout == "rm":
            B0, B1 = self.cached(("B", dtype, h, n, pad), lambda: self.split(src, dtype, pad) if on_a else (self.padded(src, dtype, pad), None))
            make = lambda: {"C": self.nan((rows_out, n + pad), dtype)}
        else:
            def cm():
                parts = (src[pat.lo:pat.hi], src[pat.remote]) if (on_a and pat.remote.size) else (src, None)
                out = []
                for part in parts:
                    if part is None:
                        out.append(None)
                        continue
                    t = self.torch.zeros((n, part.shape[0] + pad), dtype=self.TD[dtype], device=self.gpu)
                    t[:, :part.shape[0]] = self.dev(np.ascontiguousarray(part.T))
                    out.append(t)
                return tuple(out)
            B0, B1 = self.cached(("Bcm", h, n, pad), cm)
            make = lambda: {"C": self.nan((n, rows_out + pad), dtype)}

        def launch(A, At, outs):
            H = A if on_a else At
            Cd = outs["C"]
            if layout == "cm":
                hip.spmm_csr(H, B0, Cd, n=n, layout=1, B1=B1, variant=variant)
            elif dtype == "f64":
                hip.spmm_csr(H, B0, Cd[:, :n] if pad else Cd, n=n, B1=B1, variant=variant)
            else:
                hip.spmm_csr_f32(H, B0, Cd[:, :n] if pad else Cd, n=n, B1=B1, variant=variant)

        def check(outs, what):
            got = outs["C"]
            if layout == "rm":
                body, padding = got[:, :n], got[:, n:]
            else:
                body, padding = np.ascontiguousarray(got[:, :rows_out].T), got[:, rows_out:]
            assert np.isnan(padding).all(), (what, "padding written")
            vs = CP.ValueSet(snap.kind, None, snap.val)
            cur = data.sets[[i for i, s in enumerate(data.sets) if s.val is snap.val][0]]
            if on_a:
                body = self.named_rows(body, snap, what)
                want = data.product(cur, n) if cur.kind != "R" else None
                _check_product(dtype, vs.kind, pat.rp, pat.gcol, snap.val, src, want, body, what)
            else:
                want = data.product_t(cur, n) if cur.kind != "R" else None
                _check_product(dtype, vs.kind, pat.rpt, pat.cit, snap.val[pat.tmap], src, want, body, what)
        return make, launch, check, False

    def _sddmm(self, step, snap):
        _, _, dtype, mode, n, use_pos = step
        data, pat = self.data, self.pat
        X = self.cached(("X", dtype, n, id(snap.rowmap)), lambda: self.mapped(data.X[:, :n], dtype, snap))
        Y0, Y1 = self.cached(("Y", dtype, n), lambda: self.split(data.Y[:, :n], dtype))
        nnz = pat.gcol.size
        make = lambda: {"out": self.nan((nnz + CP.OUT_EXTRA if use_pos else nnz,), dtype)}

        def launch(A, At, outs):
            A.sddmm(X, Y0, Y1=Y1, out=outs["out"], out_pos=self.pos_dev if use_pos else None, mode=mode)

        def check(outs, what):
            got = self.named_pos(outs["out"], self.pos_np if use_pos else None, what)
            cur = data.sets[[i for i, s in enumerate(data.sets) if s.val is snap.val][0]]
            want = data.sddmm(cur, mode, n) if (mode == 0 or cur.kind != "R") else None
            _check_sddmm(dtype, snap.kind, mode, data, snap.val, want, n, got, what)
        return make, launch, check, False

    def _attention_operands(self, dtype, nk, nv, snap):
        data = self.data
        Q = self.cached(("Q", dtype, nk, id(snap.rowmap)), lambda: self.mapped(data.Q[:, :nk], dtype, snap))
        K0, K1 = self.cached(("K", dtype, nk), lambda: self.split(data.K[:, :nk], dtype))
        V0, V1 = self.cached(("V", dtype, nv), lambda: self.split(data.V[:, :nv], dtype))
        return Q, K0, K1, V0, V1

    def _attn(self, step, snap):
        _, _, dtype, bias, widx, use_pos = step
        nk, nv = CP.ATTN_WIDTHS[widx]
        pat = self.pat
        nnz = pat.gcol.size
        Q, K0, K1, V0, V1 = self._attention_operands(dtype, nk, nv, snap)
        scale = 1.0 / np.sqrt(nk)
        make = lambda: {"O": self.nan((snap.c_nrow, nv + 3), dtype), "lse": self.nan((snap.c_nrow,), dtype),
                        "p": self.nan((nnz + CP.OUT_EXTRA if use_pos else nnz,), dtype)}

        def launch(A, At, outs):
            A.attention(Q, K0, V0, K1=K1, V1=V1, scale=scale, bias=bias, out=outs["O"][:, :nv], lse=outs["lse"], p_out=outs["p"],
                        out_pos=self.pos_dev if use_pos else None)

        def check(outs, what):
            assert np.isnan(outs["O"][:, nv:]).all(), (what, "padding written")
            O = self.named_rows(outs["O"][:, :nv], snap, what)
            lse = self.named_rows(outs["lse"], snap, what)
            p = self.named_pos(outs["p"], self.pos_np if use_pos else None, what)
            _check_attention(dtype, self.attention_ref(dtype, bias, nk, nv, snap, snap.val), O, lse, p, what)
        return make, launch, check, True

    def _bwd(self, step, snap, with_kv):
        dtype, bias, widx = step[2], step[3], step[4]
        use_pos = step[5] if not with_kv else False
        nk, nv = CP.ATTN_WIDTHS[widx]
        pat, data, torch = self.pat, self.data, self.torch
        nnz = pat.gcol.size
        Q, K0, K1, V0, V1 = self._attention_operands(dtype, nk, nv, snap)
        dO = self.cached(("dO", dtype, nv, id(snap.rowmap)), lambda: self.mapped(data.dO[:, :nv], dtype, snap))
        scale = 1.0 / np.sqrt(nk)
        if with_kv:         # A^T's handle takes one source and A's rows in A's order
            Kp = self.cached(("Kp", dtype, nk), lambda: self.dev(data.K[:, :nk].astype(NP[dtype])))
            Vp = self.cached(("Vp", dtype, nv), lambda: self.dev(data.V[:, :nv].astype(NP[dtype])))
            Qp = self.cached(("Qp", dtype, nk), lambda: self.dev(data.Q[:, :nk].astype(NP[dtype])))
            dOp = self.cached(("dOp", dtype, nv), lambda: self.dev(data.dO[:, :nv].astype(NP[dtype])))
            idx = None if snap.rowmap is None else self.cached(("idx", id(snap.rowmap)), lambda: self.dev(snap.rowmap.astype(np.int64)))

        def make():
            outs = {"O": self.nan((snap.c_nrow, nv), dtype), "lse": self.nan((snap.c_nrow,), dtype),
                    "dQ": self.nan((snap.c_nrow, nk + 3), dtype), "delta": self.nan((snap.c_nrow,), dtype),
                    "ds": self.nan((nnz + CP.OUT_EXTRA if use_pos else nnz,), dtype)}
            if with_kv:
                outs.update({"dK": self.nan((pat.k, nk + 1), dtype), "dV": self.nan((pat.k, nv), dtype)})
            return outs

        def launch(A, At, outs):
            A.attention(Q, K0, V0, K1=K1, V1=V1, scale=scale, bias=bias, out=outs["O"], lse=outs["lse"])
            A.attention_bwd_q(Q, K0, V0, outs["O"], dO, outs["lse"], K1=K1, V1=V1, scale=scale, bias=bias, dQ=outs["dQ"][:, :nk],
                              delta=outs["delta"], ds_out=outs["ds"], out_pos=self.pos_dev if use_pos else None)
            if with_kv:
                lse, delta = outs["lse"], outs["delta"]
                if idx is not None:
                    lse, delta = lse.index_select(0, idx), delta.index_select(0, idx)
                At.attention_bwd_kv(Kp, Vp, Qp, dOp, lse, delta, scale=scale, bias=bias, dK=outs["dK"][:, :nk], dV=outs["dV"])

        def check(outs, what):
            dt = NP[dtype]
            assert np.isnan(outs["dQ"][:, nk:]).all(), (what, "padding written")
            got = {"dQ": self.named_rows(outs["dQ"][:, :nk], snap, what), "delta": self.named_rows(outs["delta"], snap, what),
                   "ds": self.named_pos(outs["ds"], self.pos_np if use_pos else None, what)}
            if with_kv:
                assert np.isnan(outs["dK"][:, nk:]).all(), (what, "padding written")
                got.update({"dK": outs["dK"][:, :nk], "dV": outs["dV"]})
            for k, v in got.items():
                assert np.isfinite(v).all(), (what, k, "non-finite output")
            fwd = self.attention_ref(dtype, bias, nk, nv, snap, snap.val)
            _check_attention(dtype, fwd, self.named_rows(outs["O"], snap, what), self.named_rows(outs["lse"], snap, what),
                             np.zeros(nnz, dt) if not fwd["bounded"] else fwd["p"].astype(dt), what)
            if fwd["bounded"]:
                ref = self.cached(("bref", dtype, bias, nk, nv, id(snap.val) if bias else None), lambda: BR.reference(
                    pat.rp, pat.gcol, data.Q[:, :nk].astype(dt), data.K[:, :nk].astype(dt), data.V[:, :nv].astype(dt),
                    data.dO[:, :nv].astype(dt), dt(scale), snap.val.astype(dt) if bias else None, ncol=pat.k))
                for k, w in BR.ratios(got, ref, dt).items():
                    _note("attention_bwd %s %s" % (k, dtype), w)
                    assert w <= 1, (what, "backward bound missed", k, w)
        return make, launch, check, True

    def _bwd_q(self, step, snap):
        return self._bwd(step, snap, False)

    def _bwd_kv(self, step, snap):
        return self._bwd(step, snap, True)

    def _softmax(self, step, snap, bwd=False):
        dtype = step[2]
        dt = NP[dtype]
        data, pat = self.data, self.pat
        s = self.cached(("s", dtype), lambda: self.dev(data.scores.astype(dt)))
        ref, L, T = self.cached(("sref", dtype), lambda: SR.reference_fwd(pat.rp, data.scores.astype(dt)))
        y_np = ref.astype(dt)
        if bwd:
            y = self.cached(("y", dtype), lambda: self.dev(y_np))
            dy = self.cached(("dy", dtype), lambda: self.dev(data.grads.astype(dt)))
        make = lambda: {"out": self.nan((pat.gcol.size,), dtype)}

        def launch(A, At, outs):
            if bwd:
                A.row_softmax_bwd(y, dy, out=outs["out"])
            else:
                A.row_softmax(s, out=outs["out"])

        def check(outs, what):
            got = outs["out"]
            assert np.isfinite(got).all(), (what, "non-finite output")
            if bwd:
                rb, Lb, S = SR.reference_bwd(pat.rp, y_np, data.grads.astype(dt))
                w = SR.worst(got, rb, SR.bound_bwd(y_np, data.grads.astype(dt), Lb, S, dt))[0]
            else:
                w = SR.worst(got, ref, SR.bound_fwd(ref, L, T, dt))[0]
            _note("row_softmax%s %s" % ("_bwd" if bwd else "", dtype), w)
            assert w <= 1, (what, "softmax bound missed", w)
        return make, launch, check, True

    def _softmax_bwd(self, step, snap):
        return self._softmax(step, snap, True)

    def queries(self, A, At):
        lib = A._lib
        return {"A.is_transposed": A.is_transposed, "T.is_transposed": At.is_transposed,
                "A.team2_compact": lib.crp_csr_dev_team2_compact(A.handle), "T.team2_compact": lib.crp_csr_dev_team2_compact(At.handle)}

    def run(self, steps=None):
        """execute the program (or the given prefix), compare everything; returns the device time of the steps in ms"""
        torch, prog, model = self.torch, self.prog, self.model
        steps = list(prog.steps if steps is None else steps)
        final = [("spmm", 0, "f64", "A", 1, 7, "rm", 0), ("spmm", 1, "f64", "T", 1, 7, "rm", 1)]       # the values are untouched
        plan = []
        for i, step in enumerate(steps + final):
            snap = self.snapshot()
            entry = None
            if step[0] not in ("update", "rowmap"):
                make, launch, check, replay = self.build(step, snap)
                entry = (make(), launch, check, replay, make)
            plan.append((i, step, snap, entry))
            model.apply(step)
            plan[-1] += (dict(model.queries()), model.T.last_variant if (step[0] == "spmm" and step[3] == "T") else model.A.last_variant)
        A, At = self.handles(self.data.sets[0].val, None)
        lib = A._lib
        A_WAS_REORDERED.append(lib.crp_csr_dev_reordered(A.handle) & lib.crp_csr_dev_reordered(At.handle))
        streams = Streams(lib, self.gpu)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(streams.s[0])
        streams.leave(0)
        try:
            for i, step, snap, entry, queries, last_variant in plan:
                try:
                    s = streams.enter(step[1])
                    with torch.cuda.stream(s):
                        if step[0] == "update":
                            for H, src in ((A, step[2]), (At, step[3])):
                                H.update_values(self.data.sets[step[4]].val if src == "host" else self.vals_dev[step[4]], stream=s.cuda_stream)
                        elif step[0] == "rowmap":
                            A.set_rowmap(*((None, 0) if step[2] == 0 else self.data.rowmaps[step[2]]))
                        else:
                            entry[1](A, At, entry[0])
                    streams.leave(step[1])
                    assert self.queries(A, At) == queries, ("queries", self.queries(A, At), "the model says", queries)
                    if step[0] == "spmm" and step[6] == "rm":
                        got = lib.crp_csr_dev_last_variant((At if step[3] == "T" else A).handle)
                        assert got == last_variant, ("the product launched variant %d, the model says %d" % (got, last_variant))
                except Exception as e:
                    raise AssertionError(self.report(i, step, steps, "while issuing", e)) from e
            streams.s[0].wait_event(streams.last)
            t1.record(streams.s[0])
            torch.cuda.synchronize()                            # the ONE synchronisation
            ms = t0.elapsed_time(t1)
            for i, step, snap, entry, _, _ in plan:
                if entry is None:
                    continue
                try:
                    entry[2]({k: v.cpu().numpy() for k, v in entry[0].items()}, (prog.seed, i, step))
                except Exception as e:
                    raise AssertionError(self.report(i, step, steps, "wrong result", e)) from e
            # the attention family once more, each call on a fresh pair of handles made from the values the model held
            for i, step, snap, entry, _, _ in plan:
                if entry is None or not entry[3]:
                    continue
                fA, fAt = self.handles(snap.val, snap)
                fresh = entry[4]()
                entry[1](fA, fAt, fresh)
                torch.cuda.synchronize()
                try:
                    _same_bits({k: v.cpu().numpy() for k, v in entry[0].items()}, {k: v.cpu().numpy() for k, v in fresh.items()}, (prog.seed, i, step))
                except Exception as e:
                    raise AssertionError(self.report(i, step, steps, "wrong result", e)) from e
                finally:
                    fA.free()
                    fAt.free()
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
        return "program seed %d (%s), %s at step %d %r: %s\n%s" % (self.prog.seed, self.prog.matrix, how, i, step, e, CP.literal(shown, i))


def _run_handle_program(gpu, monkeypatch, prog, steps=None):
    if prog.panel_order is not None:
        monkeypatch.setenv("CRPSPMM_PANEL_ORDER", prog.panel_order)
    else:
        monkeypatch.delenv("CRPSPMM_PANEL_ORDER", raising=False)
    monkeypatch.delenv("CRPSPMM_TEAM2R", raising=False)
    if prog.matrix in CP.REORDERED:
        monkeypatch.setenv("CRPSPMM_REORDER", "1")
    else:
        monkeypatch.delenv("CRPSPMM_REORDER", raising=False)
    t = time.perf_counter()
    ms = HandleRun(prog, gpu).run(steps)
    print("handle program %d (seed %d, %s%s): %d steps, %.1f ms on the device, %.2f s in all; worst error / bound so far: %s"
          % (prog.index, prog.seed, prog.matrix, ", two sources" if prog.two_source else "", len(prog.steps if steps is None else steps), ms,
             time.perf_counter() - t, ", ".join("%s %.3g" % kv for kv in sorted(WORST.items()))))


@pytest.mark.parametrize("index", range(CP.HANDLE_PROGRAMS))
def test_handle_program(crp, gpu, monkeypatch, index):
    _run_handle_program(gpu, monkeypatch, CP.handle_programs()[index])


def test_handle_program_on_reordered_rows(crp, gpu, monkeypatch):
    """the ninth program: 2048 rows under CRPSPMM_REORDER=1, so that both handles build their formats on the rows in locality order
    (f_val follows a host update, rowmap_fmt a row map, the slot maps are re-indexed by the caller's nonzeros)"""
    prog = CP.reordered_program()
    _run_handle_program(gpu, monkeypatch, prog)
    assert A_WAS_REORDERED.pop() == 1, "the handle kept the caller's order"


# ---- the engines, in process -----------------------------------------------------------------------------------------------------

class EngineRun(Base):
    """RpSpmm or Para2dSpmm (1 x 1) over comm.SelfComm"""

    def __init__(self, which, prog, n, gpu):
        self.which, self.prog, self.n = which, prog, n
        pat, data, self.model = CP.engine_setup(prog, n)
        super().__init__(gpu, data)
        self.vals_dev = {"f64": [self.dev(vs.val) for vs in data.sets], "f32": [self.dev(vs.val.astype(np.float32)) for vs in data.sets]}

    def engine(self):
        from crp_spmm_amd import comm, engine
        pat = self.pat
        self.comm = comm.SelfComm()
        val = self.data.sets[0].val
        if self.which == "rp":
            e = engine.RpSpmm(0, pat.m, pat.rp, pat.gcol, val, [0, pat.k], self.n, self.comm)
            return e, e
        e2 = engine.Para2dSpmm(self.comm, 1, 1, [0, pat.m], [0, pat.k], [0, pat.m], [0, self.n], pat.rp, pat.gcol, val)
        return e2, e2.rp

    def snapshot(self):
        return Snapshot(self.model.kind(), self.model.current_values(), None, self.pat.m)

    def current_set(self):
        return self.data.sets[self.model.cur]

    def operand(self, name, a, dtype, where, layout):
        """a dense operand as the engine takes it: layout 1 as an (n, rows) array holding the column-major data"""
        def make():
            x = np.array((a.T if layout else a).astype(NP[dtype]), order="C")
            return self.dev(x) if where == "dev" else x
        return self.cached((name, dtype, where, layout), make)

    def result(self, rows, dtype, where, layout):
        n = self.n
        if where == "host":
            return np.full((n, rows) if layout else (rows, n), np.nan, NP[dtype])
        return self.nan((n, rows + 3) if layout else (rows, n + 3), dtype)

    @staticmethod
    def body(got, rows, n, layout, what):
        """(the result as rows x n, after the padding was seen to hold NaN)"""
        if layout:
            assert np.isnan(got[:, rows:]).all(), (what, "padding written")
            return np.ascontiguousarray(got[:, :rows].T)
        assert np.isnan(got[:, n:]).all(), (what, "padding written")
        return np.ascontiguousarray(got[:, :n])

    # every builder returns (make outputs, launch(e, rp, outs, stream), check(outs as numpy), the same call on device handles or None)
    def build(self, step, snap):
        return getattr(self, "_" + step[0])(step, snap)

    def _product(self, step, snap, transposed):
        _, _, dtype, where, layout = step
        pat, data, n = self.pat, self.data, self.n
        src, rows = (data.Bt[:, :n], pat.k) if transposed else (data.B[:, :n], pat.m)
        B = self.operand("Bt" if transposed else "B", src, dtype, where, layout)
        cur = self.current_set()
        want = None if cur.kind == "R" else (data.product_t(cur, n) if transposed else data.product(cur, n))
        make = lambda: {"C": self.result(rows, dtype, where, layout)}

        def launch(e, rp, outs, stream):
            Cd = outs["C"]
            view = Cd if where == "host" else (Cd[:, :rows] if layout else Cd[:, :n])
            if transposed:
                (e.exec_t if dtype == "f64" else e.exec_t_f32)(layout, B, view, stream=stream)
            else:
                e.exec(layout, B, view, stream=stream)

        def check(outs, what):
            got = self.body(outs["C"], rows, n, layout, what)
            if transposed:
                _check_product(dtype, snap.kind, pat.rpt, pat.cit, snap.val[pat.tmap], src, want, got, what)
            else:
                _check_product(dtype, snap.kind, pat.rp, pat.gcol, snap.val, src, want, got, what)
        return make, launch, check, None

    def _exec(self, step, snap):
        return self._product(step, snap, False)

    def _exec_t(self, step, snap):
        return self._product(step, snap, True)

    def _sddmm(self, step, snap):
        _, _, dtype, mode, where = step                 # where: X, Y and out all on the device or all on the host
        pat, data, n = self.pat, self.data, self.n
        X, Y = self.operand("X", data.X[:, :n], dtype, where, 0), self.operand("Y", data.Y[:, :n], dtype, where, 0)
        cur = self.current_set()
        want = data.sddmm(cur, mode, n) if (mode == 0 or cur.kind != "R") else None
        nnz = pat.gcol.size
        make = lambda: {"out": np.full(nnz, np.nan, NP[dtype]) if where == "host" else self.nan((nnz,), dtype)}

        def launch(e, rp, outs, stream):
            e.sddmm(0, X, Y, outs["out"], mode=mode, stream=stream)

        def check(outs, what):
            _check_sddmm(dtype, snap.kind, mode, data, snap.val, want, n, outs["out"], what)
        return make, launch, check, None

    def _attn(self, step, snap, bwd=False):
        _, _, dtype, bias = step
        pat, data, n = self.pat, self.data, self.n
        dt = NP[dtype]
        nnz = pat.gcol.size
        Q, K, V, dO = (self.operand(k, getattr(data, k)[:, :n], dtype, "dev", 0) for k in ("Q", "K", "V", "dO"))
        scale = 1.0 / np.sqrt(n)

        def make():
            outs = {"O": self.nan((pat.m, n + 3), dtype), "lse": self.nan((pat.m,), dtype), "p": self.nan((nnz,), dtype)}
            if bwd:
                outs.update({"dQ": self.nan((pat.m, n + 1), dtype), "dK": self.nan((pat.k, n + 2), dtype), "dV": self.nan((pat.k, n), dtype),
                             "ds": self.nan((nnz,), dtype)})
            return outs

        def launch(e, rp, outs, stream):
            e.attention(0, Q, K, V, outs["O"][:, :n], scale=scale, bias=bias, lse=outs["lse"], p_out=outs["p"], stream=stream)
            if bwd:
                e.attention_bwd(Q, K, V, outs["O"][:, :n], dO, outs["lse"], outs["dQ"][:, :n], outs["dK"][:, :n], outs["dV"], scale=scale,
                                bias=bias, ds_out=outs["ds"], stream=stream)

        def handle_call(A, At, outs):
            """the same on a pair of device handles (include/crp_engine.h: the engine's results equal them at one rank)"""
            A.attention(Q, K, V, scale=scale, bias=bias, out=outs["O"][:, :n], lse=outs["lse"], p_out=outs["p"])
            if bwd:
                delta = self.nan((pat.m,), dtype)
                A.attention_bwd_q(Q, K, V, outs["O"][:, :n], dO, outs["lse"], scale=scale, bias=bias, dQ=outs["dQ"][:, :n], delta=delta,
                                  ds_out=outs["ds"])
                At.attention_bwd_kv(K, V, Q, dO, outs["lse"], delta, scale=scale, bias=bias, dK=outs["dK"][:, :n], dV=outs["dV"])

        def check(outs, what):
            fwd = self.attention_ref(dtype, bias, n, n, snap, snap.val)
            for k in ("O", "dQ", "dK"):
                if k in outs:
                    assert np.isnan(outs[k][:, n:]).all(), (what, "padding written")
            _check_attention(dtype, fwd, outs["O"][:, :n], outs["lse"], outs["p"], what)
            if bwd:
                got = {"dQ": outs["dQ"][:, :n], "dK": outs["dK"][:, :n], "dV": outs["dV"], "ds": outs["ds"]}
                for k, v in got.items():
                    assert np.isfinite(v).all(), (what, k, "non-finite output")
                if fwd["bounded"]:
                    ref = self.cached(("bref", dtype, bias, id(snap.val) if bias else None), lambda: BR.reference(
                        pat.rp, pat.gcol, data.Q[:, :n].astype(dt), data.K[:, :n].astype(dt), data.V[:, :n].astype(dt), data.dO[:, :n].astype(dt),
                        dt(scale), snap.val.astype(dt) if bias else None, ncol=pat.k))
                    for k, w in BR.ratios(got, ref, dt).items():
                        _note("attention_bwd %s %s" % (k, dtype), w)
                        assert w <= 1, (what, "backward bound missed", k, w)
        return make, launch, check, handle_call

    def _attn_bwd(self, step, snap):
        return self._attn(step, snap, True)

    def _softmax(self, step, snap, bwd=False):
        dtype = step[2]
        dt = NP[dtype]
        data, pat = self.data, self.pat
        s = self.cached(("s", dtype), lambda: self.dev(data.scores.astype(dt)))
        ref, L, T = self.cached(("sref", dtype), lambda: SR.reference_fwd(pat.rp, data.scores.astype(dt)))
        y_np = ref.astype(dt)
        y = self.cached(("y", dtype), lambda: self.dev(y_np))
        dy = self.cached(("dy", dtype), lambda: self.dev(data.grads.astype(dt)))
        make = lambda: {"out": self.nan((pat.gcol.size,), dtype)}

        def launch(e, rp, outs, stream):
            if bwd:
                e.row_softmax_bwd(y, dy, out=outs["out"], stream=stream)
            else:
                e.row_softmax(s, out=outs["out"], stream=stream)

        def handle_call(A, At, outs):
            if bwd:
                A.row_softmax_bwd(y, dy, out=outs["out"])
            else:
                A.row_softmax(s, out=outs["out"])

        def check(outs, what):
            got = outs["out"]
            assert np.isfinite(got).all(), (what, "non-finite output")
            if bwd:
                rb, Lb, S = SR.reference_bwd(pat.rp, y_np, data.grads.astype(dt))
                w = SR.worst(got, rb, SR.bound_bwd(y_np, data.grads.astype(dt), Lb, S, dt))[0]
            else:
                w = SR.worst(got, ref, SR.bound_fwd(ref, L, T, dt))[0]
            _note("row_softmax%s %s" % ("_bwd" if bwd else "", dtype), w)
            assert w <= 1, (what, "softmax bound missed", w)
        return make, launch, check, handle_call

    def _softmax_bwd(self, step, snap):
        return self._softmax(step, snap, True)

    def queries(self, e, rp):
        q = {"transposed_built": rp.transposed_built, "sddmm_built": rp.sddmm_built, "attention_built": rp.attention_built(),
             "attention_bwd_built": rp.attention_bwd_built(), "row_softmax_built": rp.row_softmax_built,
             "host_values_stale": rp.host_values_stale}
        if e is not rp:
            assert e.row_softmax_built == rp.row_softmax_built and not e.sddmm_built         # (1 x 1: the row engine's; no grid-row buffers)
        return q

    def run(self, steps=None):
        from crp_spmm_amd import hip
        torch, prog, model, pat = self.torch, self.prog, self.model, self.pat
        steps = list(prog.steps if steps is None else steps)
        final = [("set_variant", 0, 1), ("exec", 1, "f64", "dev", 0)]                   # the values are untouched
        control = ("update", "update_dev", "set_variant", "set_variant_f32", "set_timing")
        plan = []
        for i, step in enumerate(steps + final):
            snap = self.snapshot()
            entry = None
            if step[0] not in control:
                make, launch, check, handle_call = self.build(step, snap)
                entry = (make(), launch, check, handle_call, make)
            model.apply(step)
            plan.append((i, step, snap, entry, dict(model.queries())))
        e, rp = self.engine()
        streams = Streams(e._lib, self.gpu)
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
                            e.update_values(self.data.sets[step[2]].val)
                        elif step[0] == "update_dev":
                            e.update_values_dev(self.vals_dev[step[3]][step[2]], stream=s.cuda_stream)
                        elif step[0] == "set_variant":
                            rp.set_variant(step[2])
                        elif step[0] == "set_variant_f32":
                            rp.set_variant_f32(step[2])
                        elif step[0] == "set_timing":
                            rp.set_timing(step[2])
                        else:
                            entry[1](e, rp, entry[0], s.cuda_stream)
                    streams.leave(step[1])
                    got = self.queries(e, rp)
                    assert got == queries, ("queries", got, "the model says", queries)
                except Exception as ex:
                    raise AssertionError(self.report(i, step, steps, "while issuing", ex)) from ex
            streams.s[0].wait_event(streams.last)
            t1.record(streams.s[0])
            torch.cuda.synchronize()                            # the ONE synchronisation
            ms = t0.elapsed_time(t1)
            host = lambda outs: {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in outs.items()}
            for i, step, snap, entry, _ in plan:
                if entry is None:
                    continue
                try:
                    entry[2](host(entry[0]), (prog.seed, i, step))
                except Exception as ex:
                    raise AssertionError(self.report(i, step, steps, "wrong result", ex)) from ex
            # the attention family once more, as the device handle calls on a fresh pair of handles made from the model's values
            for i, step, snap, entry, _ in plan:
                if entry is None or entry[3] is None:
                    continue
                fA = hip.CsrDev(pat.m, pat.k, pat.rp, pat.gcol, snap.val)
                fAt = hip.CsrDev.from_transpose(pat.m, pat.k, pat.rp, pat.gcol, snap.val)
                fresh = entry[4]()
                entry[3](fA, fAt, fresh)
                torch.cuda.synchronize()
                try:
                    _same_bits(host(entry[0]), host(fresh), (prog.seed, i, step))
                except Exception as ex:
                    raise AssertionError(self.report(i, step, steps, "wrong result", ex)) from ex
                finally:
                    fA.free()
                    fAt.free()
        finally:
            torch.cuda.synchronize()
            e.free()
            streams.close()
            self.comm.free()
        return ms

    def report(self, i, step, steps, how, e):
        shown = self.prog._replace(steps=tuple(steps))
        head = "%s program seed %d (%s, glb_n %d)" % (self.which, self.prog.seed, self.prog.matrix, self.n)
        if i >= len(steps):
            return "%s, %s at the closing variant-1 product %r after all %d steps: %s" % (head, how, step, len(steps), e)
        return "%s, %s at step %d %r: %s\n%s" % (head, how, i, step, e, CP.literal(shown, i))


def _run_engine_program(gpu, monkeypatch, which, index, steps=None):
    for k in ("CRPSPMM_PANEL_ORDER", "CRPSPMM_TEAM2R"):
        monkeypatch.delenv(k, raising=False)
    prog, n = CP.engine_programs(which)[index]
    t = time.perf_counter()
    ms = EngineRun(which, prog, n, gpu).run(steps)
    print("%s program %d (seed %d, %s, glb_n %d): %d steps, %.1f ms on the device, %.2f s in all; worst error / bound so far: %s"
          % (which, index, prog.seed, prog.matrix, n, len(prog.steps if steps is None else steps), ms, time.perf_counter() - t,
             ", ".join("%s %.3g" % kv for kv in sorted(WORST.items()))))


@pytest.mark.parametrize("index", range(CP.ENGINE_PROGRAMS["rp"]))
def test_rp_engine_program(crp, gpu, monkeypatch, index):
    _run_engine_program(gpu, monkeypatch, "rp", index)


@pytest.mark.parametrize("index", range(CP.ENGINE_PROGRAMS["para2d"]))
def test_para2d_engine_program(crp, gpu, monkeypatch, index):
    _run_engine_program(gpu, monkeypatch, "para2d", index)

