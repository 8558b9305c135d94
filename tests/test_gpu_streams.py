"""GPU: the stream contract of include/crpspmm_hip.h ("Streams") and include/crp_engine.h, on a held-back non-blocking side
stream (tests/streams_harness.py, which explains the method).  Measured on the MI355X: the slowest steady-state host call of the
table is hip.sparse_attention forward + backward at 0.52 ms, the delay is 120 ms (2.39e6 cycles of torch.cuda._sleep per ms).

TABLE reaches every launcher of the device ABI at least once, on the smallest matrix that reaches it; the kernels' numerics are
pinned elsewhere.  Every row makes three assertions -- Order, Asynchrony, Control -- and every row that is not `blocking` is also
captured into a graph on the side stream and replayed on a second data set.

Order is asserted BIT FOR BIT in every row: the header promises repeatability for every call of the table (crp_spmm_csr_f64:
"repeated calls are bit-identical"; crp_sddmm_csr_*, the row softmax, crp_scatter_add_rows_*, crp_sum_segments_*: "Repeated calls
are ... bit-identical"; the attention calls and their backward: "A row's bits depend on (dtype, nk, nv, scale, bias) and the row's
entries in CSR order ONLY"; the fp32 products are pinned exactly by tests/test_gpu_fp32_kernels.py; the row movers only move), so
no row falls back to a bound.

BLOCKING holds the only calls that may block, each with the header sentence that says so (test_blocking_rows_quote_the_header);
they are exempt from Asynchrony and are the calls that are not capturable (NOT_CAPTURABLE is the same table: nothing else is in it).

The engines (world 1, timing off) run the same way, then the cross-stream orderings INTEGRATION.md documents are pinned: each is
deterministic thanks to the hold-back, and only values differ when one is violated.  World 2: tests/gpu_dist_streams_worker.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import streams_harness as H
from conftest import ROOT

pytestmark = pytest.mark.gpu

M, K = 500, 300                      # gen.random_csr(500, 300, 30, empty_every=13)
HALF = 150                           # the two-source handle: columns >= HALF are rows of the second source

# the header's sentences (include/crpspmm_hip.h, "Streams"; include/crp_engine.h), whitespace-normalised
BLOCKING = {
    "host-values": "With a host pointer crp_csr_dev_update_values blocks until the values have left the caller's array.",
    "csr-transpose": "HIP kernels on `stream`, which the call synchronises",
    "first-build": "The first call that builds state on a handle blocks: what it builds is complete on return.",
    "timing-on": "With timing on every call waits for its stream.",
}
NOT_CAPTURABLE = BLOCKING


def test_blocking_rows_quote_the_header():
    text = ""
    for name in ("crpspmm_hip.h", "crp_engine.h"):
        with open(os.path.join(ROOT, "include", name)) as f:
            text += re.sub(r"[\s*/]+", " ", f.read())
    for key, sentence in BLOCKING.items():
        assert re.sub(r"[\s*/]+", " ", sentence) in text, key
    assert all(b is None or b in BLOCKING for _, b, _ in TABLE)


class Ctx:
    """what the rows share: the device, the library, the held-back stream, the matrices and handles (made on first use)"""

    def __init__(self, crp, gpu):
        from crp_spmm_amd import gen
        self.crp, self.gpu, self.lib = crp, gpu, crp.load()
        self.held = H.Held(self.lib)
        self.rp, self.ci, self.va = gen.random_csr(M, K, 30, empty_every=13)
        self.va2 = np.random.default_rng(8).uniform(-2, 2, self.ci.size)
        self.cache, self.keep = {}, []
        self.kernels = set()

    def handle(self, key):
        from crp_spmm_amd import hip
        import attention_bwd_ref as B
        if key not in self.cache:
            if key in ("A", "A-upd"):
                h = hip.CsrDev(M, K, self.rp, self.ci, self.va)
            elif key == "At-upd":
                h = hip.CsrDev.from_transpose(M, K, self.rp, self.ci, self.va)
            elif key == "A2":                                     # two-source column codes
                ci2 = np.where(self.ci >= HALF, ~(self.ci - HALF), self.ci).astype(np.int32)
                h = hip.CsrDev(M, HALF, self.rp, ci2, self.va)
            else:
                rp, ci, nrow = B.matrix()
                va = np.random.default_rng(3).uniform(-1, 1, ci.size)
                h = (hip.CsrDev if key == "B" else hip.CsrDev.from_transpose)(nrow, B.NCOL, rp, ci, va)
            self.cache[key] = h
        return self.cache[key]

    def close(self):
        self.held.close()
        for h in list(self.cache.values()) + self.keep:
            h.free()


@pytest.fixture(scope="module")
def ctx(crp, gpu):
    c = Ctx(crp, gpu)
    yield c
    c.close()


def _tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def _rnd(seed, shape, dt=np.float64):
    return np.random.default_rng(seed).standard_normal(shape).astype(dt)


def _cur(stream):
    """the stream argument of a raw library call: torch's current stream unless the control names the null stream"""
    import torch
    return torch.cuda.current_stream().cuda_stream if stream is None else (stream or None)


# ---- the rows: a builder takes the Ctx and returns (Operands, call(stream)) --------------------------------------------------

def _spmm(variant, n, launcher, layout=0, fresh=False):
    def build(c):
        from crp_spmm_amd import hip
        ops = H.Operands(c.gpu)
        import torch
        if layout == 0:
            B, C = ops.dense(_rnd(1, (K, n))), ops.out((M, n), torch.float64)
        else:
            B, C = ops.dense(_rnd(1, (n, K))), ops.out((n, M), torch.float64)

        def call(stream):
            A = c.handle("A")
            if fresh:                                             # the first product of a new handle: it builds the format
                A = hip.CsrDev(M, K, c.rp, c.ci, c.va)
                c.keep.append(A)
            hip.spmm_csr(A, B, C, n=n, layout=layout, variant=variant, stream=stream)
            assert A.last_kernel.startswith(launcher), (A.last_kernel, launcher)
            c.kernels.add(launcher)
        return ops, call
    return build


def _spmm_f32(variant, n, launcher, fresh=False):
    def build(c):
        from crp_spmm_amd import hip
        import torch
        ops = H.Operands(c.gpu)
        B, C = ops.dense(_rnd(2, (K, n), np.float32)), ops.out((M, n), torch.float32)

        def call(stream):
            A = c.handle("A")
            if fresh:
                A = hip.CsrDev(M, K, c.rp, c.ci, c.va)
                c.keep.append(A)
            hip.spmm_csr_f32(A, B, C, variant=variant, stream=stream)
            assert A.last_kernel.startswith(launcher), (A.last_kernel, launcher)
            c.kernels.add(launcher)
        return ops, call
    return build


def _sddmm(dt, mode, two_source=False, out_pos=False):
    def build(c):
        import torch
        n = 24
        ops = H.Operands(c.gpu)
        A = c.handle("A2" if two_source else "A")
        X = ops.dense(_rnd(3, (M, n), dt))
        Y0 = ops.dense(_rnd(4, (HALF if two_source else K, n), dt))
        Y1 = ops.dense(_rnd(5, (K - HALF, n), dt)) if two_source else None
        out = ops.out((A.nnz,), _tdt(dt))
        pos = torch.from_numpy(np.random.default_rng(6).permutation(A.nnz).astype(np.int32)).to(c.gpu) if out_pos else None
        return ops, lambda stream: A.sddmm(X, Y0, Y1, out=out, out_pos=pos, mode=mode, stream=stream)
    return build


def _attn_data(c, dt, seed, nk=16, nv=24):
    """Q, K, V, dO and what the forward writes for them on the default stream: O, lse (staging data of the backward rows)"""
    import torch
    import attention_bwd_ref as B
    A = c.handle("B")
    Q, Kk, V, dO = (torch.from_numpy(_rnd(seed + i, sh, dt)).to(c.gpu)
                    for i, sh in enumerate(((B.NROW, nk), (B.NCOL, nk), (B.NCOL, nv), (B.NROW, nv))))
    lse = torch.empty((B.NROW,), dtype=Q.dtype, device=c.gpu)
    O = A.attention(Q, Kk, V, scale=0.25, bias=True, lse=lse)
    dQ, delta = A.attention_bwd_q(Q, Kk, V, O, dO, lse, scale=0.25, bias=True)
    torch.cuda.synchronize()
    return dict(Q=Q, K=Kk, V=V, dO=dO, O=O, lse=lse, delta=delta)


def _attention(dt):
    def build(c):
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        A = c.handle("B")
        d0, d1 = _attn_data(c, dt, 10), _attn_data(c, dt, 20)
        Q, Kk, V = (ops.dense(d0[k], d1[k]) for k in ("Q", "K", "V"))
        O, lse, p = ops.out((B.NROW, 24), _tdt(dt)), ops.out((B.NROW,), _tdt(dt)), ops.out((A.nnz,), _tdt(dt))
        return ops, lambda stream: A.attention(Q, Kk, V, scale=0.25, bias=True, out=O, lse=lse, p_out=p, stream=stream)
    return build


def _attention_bwd_q(dt):
    def build(c):
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        A = c.handle("B")
        d0, d1 = _attn_data(c, dt, 10), _attn_data(c, dt, 20)
        Q, Kk, V, O, dO, lse = (ops.dense(d0[k], d1[k]) for k in ("Q", "K", "V", "O", "dO", "lse"))
        dQ, delta, ds = ops.out((B.NROW, 16), _tdt(dt)), ops.out((B.NROW,), _tdt(dt)), ops.out((A.nnz,), _tdt(dt))
        return ops, lambda stream: A.attention_bwd_q(Q, Kk, V, O, dO, lse, scale=0.25, bias=True, dQ=dQ, delta=delta, ds_out=ds,
                                                     stream=stream)
    return build


def _attention_bwd_kv(dt, in_place=False):
    def build(c):
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        At = c.handle("Bt")
        d0, d1 = _attn_data(c, dt, 10), _attn_data(c, dt, 20)
        Kk, V = (ops.dense(d0[k], d1[k], inout=in_place) for k in ("K", "V"))
        Q, dO, lse, delta = (ops.dense(d0[k], d1[k]) for k in ("Q", "dO", "lse", "delta"))
        dK, dV = (Kk, V) if in_place else (ops.out((B.NCOL, 16), _tdt(dt)), ops.out((B.NCOL, 24), _tdt(dt)))
        return ops, lambda stream: At.attention_bwd_kv(Kk, V, Q, dO, lse, delta, scale=0.25, bias=True, dK=dK, dV=dV, stream=stream)
    return build


def _softmax(dt, bwd, raw):
    def build(c):
        import torch
        from crp_spmm_amd import hip
        ops = H.Operands(c.gpu)
        A = c.handle("A")
        nnz = A.nnz
        rowptr = torch.from_numpy(c.rp).to(c.gpu)
        s = ops.dense(_rnd(7, (nnz,), dt))
        out = ops.out((nnz,), _tdt(dt))
        if not bwd:
            if raw:
                return ops, lambda stream: hip.row_softmax(rowptr, s, out=out, stream=stream)
            return ops, lambda stream: A.row_softmax(s, out=out, stream=stream)
        dy = ops.dense(_rnd(8, (nnz,), dt))
        if raw:
            return ops, lambda stream: hip.row_softmax_bwd(rowptr, s, dy, out=out, stream=stream)
        return ops, lambda stream: A.row_softmax_bwd(s, dy, out=out, stream=stream)
    return build


def _update_then_product(transposed, host=False):
    """new values (a device tensor; host: a numpy array, the blocking form), then a product on the row-panel format they refresh"""
    def build(c):
        import torch
        from crp_spmm_amd import hip
        n = 64
        ops = H.Operands(c.gpu)
        A = c.handle("At-upd" if transposed else "A-upd")
        vals = c.va2 if host else ops.dense(c.va2, 0.5 * c.va)
        B, C = ops.dense(_rnd(9, (A.ncol, n))), ops.out((A.nrow, n), torch.float64)

        def call(stream):
            A.update_values(vals, stream=stream)
            hip.spmm_csr(A, B, C, variant=3, stream=stream)
        return ops, call
    return build


def _move(what, dt):
    def build(c):
        import torch
        from crp_spmm_amd import hip
        ops = H.Operands(c.gpu)
        n, nidx = 10, 120
        f32 = np.dtype(dt) == np.float32
        ridx = torch.from_numpy(np.random.default_rng(1).permutation(K)[:nidx].astype(np.int32)).to(c.gpu)
        if what == "transpose":
            src, dst = ops.dense(_rnd(11, (37, 65), dt)), ops.out((65, 37), _tdt(dt))
            fn = hip.transpose_f32 if f32 else hip.transpose
            return ops, lambda stream: fn(src, dst, stream=stream)
        if what == "gather":
            src, dst = ops.dense(_rnd(12, (K, n), dt)), ops.out((nidx, n), _tdt(dt))
            if f32:
                return ops, lambda stream: hip.gather_rows_f32(ridx, src, dst, stream=stream)
            return ops, lambda stream: hip.gather_rows(ridx, src, dst, stream=stream)
        src, dst = ops.dense(_rnd(13, (nidx, n), dt)), ops.out((K, n), _tdt(dt))
        if f32:
            return ops, lambda stream: hip.scatter_rows_f32(ridx, src, dst, stream=stream)
        return ops, lambda stream: hip.gather_rows(ridx, src, dst, scatter=True, stream=stream)
    return build


def _helper(what, dt):
    """the device helpers without a Python wrapper: the raw library call on torch's current stream"""
    def build(c):
        import torch
        from crp_spmm_amd import _lib as L
        ops = H.Operands(c.gpu)
        sfx = "f32" if np.dtype(dt) == np.float32 else "f64"
        if what == "scatter_add_rows":
            n, nseg, nsrc = 9, 40, 100
            rng = np.random.default_rng(14)
            seg_row = torch.from_numpy(rng.permutation(64)[:nseg].astype(np.int32)).to(c.gpu)              # distinct rows
            cnt = rng.integers(0, 5, nseg)
            seg_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)).to(c.gpu)
            seg_pos = torch.from_numpy(rng.integers(0, nsrc, int(cnt.sum())).astype(np.int32)).to(c.gpu)
            src, dst = ops.dense(_rnd(15, (nsrc, n), dt)), ops.dense(_rnd(16, (64, n), dt), inout=True)
            fn = getattr(c.lib, "crp_scatter_add_rows_" + sfx)
            return ops, lambda stream: L.check(fn(nseg, n, seg_row.data_ptr(), seg_ptr.data_ptr(), seg_pos.data_ptr(), src.data_ptr(), n,
                                                  dst.data_ptr(), n, _cur(stream)), fn.__name__)
        if what == "gather_vals":
            cnt = 700
            vmap = torch.from_numpy(np.random.default_rng(17).integers(0, 500, cnt).astype(np.int32)).to(c.gpu)
            src, dst = ops.dense(_rnd(18, (500,), dt)), ops.out((cnt,), torch.float64)
            fn = c.lib.crp_gather_vals_f32_f64 if sfx == "f32" else c.lib.crp_gather_vals_f64
            return ops, lambda stream: L.check(fn(cnt, vmap.data_ptr(), src.data_ptr(), dst.data_ptr(), _cur(stream)), fn.__name__)
        nseg, ln = 3, 259
        src, out = ops.dense(_rnd(19, (nseg * ln,), dt)), ops.out((ln,), _tdt(dt))
        fn = getattr(c.lib, "crp_sum_segments_" + sfx)
        return ops, lambda stream: L.check(fn(nseg, ln, src.data_ptr(), ln, out.data_ptr(), _cur(stream)), fn.__name__)
    return build


def _sparse_attention(c):
    """hip.sparse_attention forward and .backward: no stream argument anywhere, the control makes the null stream current"""
    import torch
    from crp_spmm_amd import hip
    import attention_bwd_ref as B
    ops = H.Operands(c.gpu)
    A, At = c.handle("B"), c.handle("Bt")
    d0, d1 = _attn_data(c, np.float64, 10), _attn_data(c, np.float64, 20)
    Q, Kk, V, dO = (ops.dense(d0[k], d1[k]) for k in ("Q", "K", "V", "dO"))
    outs = [ops.out(sh, torch.float64) for sh in ((B.NROW, 24), (B.NROW, 16), (B.NCOL, 16), (B.NCOL, 24))]

    def run():
        q, k, v = (t.detach().requires_grad_(True) for t in (Q, Kk, V))
        O = hip.sparse_attention(A, At, q, k, v, scale=0.25, bias=True)
        grads = torch.autograd.grad(O, (q, k, v), dO)
        for dst, src in zip(outs, (O.detach(),) + tuple(grads)):
            dst.copy_(src)

    def call(stream):
        if stream is None:
            return run()
        with torch.cuda.stream(torch.cuda.default_stream()):
            run()
    return ops, call


def _csr_transpose(c):
    import torch
    from crp_spmm_amd import hip
    ops = H.Operands(c.gpu)
    rowptr, colidx = torch.from_numpy(c.rp).to(c.gpu), torch.from_numpy(c.ci).to(c.gpu)
    val = ops.dense(c.va)
    val_t = ops.out((c.ci.size,), torch.float64)

    def call(stream):
        val_t.copy_(hip.csr_transpose(rowptr, colidx, val, K, stream=None if stream is None else 0)[2])
    return ops, call


F64, F32 = np.float64, np.float32
TABLE = [("spmm_csr-v%d-n%d" % (v, n), None, _spmm(v, n, k_))
         for v, n, k_ in ((1, 24, "rowgroup<"), (1, 64, "rowgroup<"), (1, 256, "rowgroup<"),
                          (2, 24, "panel<4"), (2, 64, "panel<4"), (2, 256, "panel<4"),
                          (3, 24, "narrow<"), (3, 64, "panel<8"), (3, 256, "panel<8"),
                          (5, 24, "team2<f64"), (5, 64, "team2<f64"), (5, 256, "team2<f64"),
                          (7, 24, "team2r<4"), (7, 64, "team2r<2"), (7, 256, "panel<8"))]
TABLE += [("spmm_csr-column-major", None, _spmm(0, 24, "cm", layout=1)),
          ("spmm_csr_f32-v1", None, _spmm_f32(1, 64, "rowgroup_f32<")),
          ("spmm_csr_f32-v5", None, _spmm_f32(5, 64, "team2<f32"))]
TABLE += [("sddmm-%s-mode%d" % (np.dtype(dt).name, mode), None, _sddmm(dt, mode)) for dt in (F64, F32) for mode in (0, 1)]
TABLE += [("sddmm-two-source-%s" % np.dtype(dt).name, None, _sddmm(dt, 1, two_source=True, out_pos=True)) for dt in (F64, F32)]
TABLE += [("attention-%s" % np.dtype(dt).name, None, _attention(dt)) for dt in (F64, F32)]
TABLE += [("attention_bwd_q-%s" % np.dtype(dt).name, None, _attention_bwd_q(dt)) for dt in (F64, F32)]
TABLE += [("attention_bwd_kv-%s" % np.dtype(dt).name, None, _attention_bwd_kv(dt)) for dt in (F64, F32)]
TABLE += [("attention_bwd_kv-in-place-%s" % np.dtype(dt).name, None, _attention_bwd_kv(dt, in_place=True)) for dt in (F64, F32)]
TABLE += [("row_softmax%s-%s-%s" % ("_bwd" if bwd else "", "raw" if raw else "handle", np.dtype(dt).name), None, _softmax(dt, bwd, raw))
          for bwd in (False, True) for raw in (True, False) for dt in (F64, F32)]
TABLE += [("update_values-device-then-product", None, _update_then_product(False)),
          ("update_values-device-then-product-from_transpose", None, _update_then_product(True))]
TABLE += [("%s-%s" % (what, np.dtype(dt).name), None, _move(what, dt)) for what in ("gather", "scatter", "transpose") for dt in (F64, F32)]
TABLE += [("%s-%s" % (what, np.dtype(dt).name), None, _helper(what, dt))
          for what in ("scatter_add_rows", "gather_vals", "sum_segments") for dt in (F64, F32)]
TABLE += [("sparse_attention-forward-backward", None, _sparse_attention)]
TABLE += [("update_values-host-then-product", "host-values", _update_then_product(False, host=True)),
          ("csr_transpose-device", "csr-transpose", _csr_transpose),
          ("first-product-builds-team2", "first-build", _spmm(5, 64, "team2<f64", fresh=True)),
          ("first-product-builds-team2r", "first-build", _spmm(7, 24, "team2r<4", fresh=True)),
          ("first-fp32-product-converts-the-values", "first-build", _spmm_f32(1, 64, "rowgroup_f32<", fresh=True)),
          ("first-fp32-team-product-converts-the-streams", "first-build", _spmm_f32(5, 64, "team2<f32", fresh=True))]
LAUNCHERS = {"rowgroup<", "cm", "panel<4", "panel<8", "narrow<", "team2r<4", "team2r<2", "team2<f64", "rowgroup_f32<", "team2<f32"}


@pytest.mark.parametrize("name,blocking,build", TABLE, ids=[t[0] for t in TABLE])
def test_order_asynchrony_control(ctx, name, blocking, build):
    ops, call = build(ctx)
    held = ctx.held
    want = held.reference(ops, call, name=None if blocking else name)
    if not blocking:
        held.warm(ops, call)
    got, pending = held.run(ops, call)
    assert H.same(got, want), "Order: the held-back call differs from the default-stream call"
    if not blocking:
        assert pending, "Asynchrony: the marker had completed when the call returned (the call waited for its stream)"
    bad, _ = held.run(ops, call, stream=0)
    held.heal(ops, call)
    assert not H.same(bad, want), "Control: a launch on the null stream went unnoticed"


@pytest.mark.parametrize("name,build", [(t[0], t[2]) for t in TABLE if t[1] is None], ids=[t[0] for t in TABLE if t[1] is None])
def test_graph_capture_and_replay(ctx, name, build):
    """one linear graph on the side stream per call: captured on data set 0, replayed on data set 1 written in place"""
    ops, call = build(ctx)
    held = ctx.held
    want = held.reference(ops, call, k=1)
    held.warm(ops, call)
    got = held.replay(ops, call)
    assert H.same(got, want), "the replay differs from the eager call on the second data set"


def test_the_table_reaches_every_launcher(ctx):
    """after the rows above (same module, same Ctx): every product launcher was named by a row"""
    if not ctx.kernels:
        for name, blocking, build in TABLE:
            if blocking is None:
                ops, call = build(ctx)
                ctx.held.reference(ops, call, name=name)
    assert LAUNCHERS <= ctx.kernels, LAUNCHERS - ctx.kernels


# ---- part D: state built by the first caller and used by later callers on other streams -------------------------------------

@pytest.mark.parametrize("variant,launcher", [(1, "rowgroup_f32<"), (5, "team2<f32")])
def test_first_fp32_product_on_one_stream_then_a_product_on_another(ctx, variant, launcher):
    """The fp32 copies of the values are built by the first fp32 product, on its stream.  First product on the held-back S1, then
    an independent product of the same handle on the free S2, nothing ordering the two: both are correct (the state a call
    builds is complete on return; without that the second product reads an unconverted copy)."""
    import torch
    from crp_spmm_amd import hip
    n = 64
    held = ctx.held
    ops = H.Operands(ctx.gpu)
    B, C1 = ops.dense(_rnd(31, (K, n), np.float32)), ops.out((M, n), torch.float32)
    B2 = torch.from_numpy(_rnd(32, (K, n), np.float32)).to(ctx.gpu)
    C2 = torch.full((M, n), H.SENTINEL, dtype=torch.float32, device=ctx.gpu)
    W = hip.CsrDev(M, K, ctx.rp, ctx.ci, ctx.va)                  # the reference: a handle of its own, on the default stream
    ctx.keep.append(W)
    ops.load(0)
    hip.spmm_csr_f32(W, B, C1, variant=variant)
    hip.spmm_csr_f32(W, B2, C2, variant=variant)
    torch.cuda.synchronize()
    assert W.last_kernel.startswith(launcher)
    want1, want2 = C1.clone(), C2.clone()
    A = hip.CsrDev(M, K, ctx.rp, ctx.ci, ctx.va)
    ctx.keep.append(A)
    if variant == 5:
        hip.spmm_csr(A, torch.from_numpy(_rnd(33, (K, n))).to(ctx.gpu), torch.empty((M, n), dtype=torch.float64, device=ctx.gpu), variant=5)
    ops.poison()
    ops.clear()
    C2.fill_(H.SENTINEL)
    torch.cuda.synchronize()
    S2 = held.second()
    with torch.cuda.stream(held.S):
        held.hold()
        ops.load(0)
        ops.clear()
        hip.spmm_csr_f32(A, B, C1, variant=variant)
    with torch.cuda.stream(S2):
        hip.spmm_csr_f32(A, B2, C2, variant=variant)
    S2.synchronize()
    held.S.synchronize()
    torch.cuda.synchronize()
    assert H.same([C2], [want2]), "the product on the second stream read state the first call had not finished building"
    assert H.same([C1], [want1])


def test_first_team2r_product_on_one_stream_then_a_product_on_another(ctx):
    """variant 7 fills the C rows of its entry table on the first product's stream: the same two-stream case, run once, after
    the fix (the stale state would be row indices)"""
    import torch
    from crp_spmm_amd import hip
    n = 24
    held = ctx.held
    ops = H.Operands(ctx.gpu)
    B, C1 = ops.dense(_rnd(41, (K, n))), ops.out((M, n), torch.float64)
    B2 = torch.from_numpy(_rnd(42, (K, n))).to(ctx.gpu)
    C2 = torch.full((M, n), H.SENTINEL, dtype=torch.float64, device=ctx.gpu)
    W = ctx.handle("A")
    ops.load(0)
    hip.spmm_csr(W, B, C1, variant=7)
    hip.spmm_csr(W, B2, C2, variant=7)
    torch.cuda.synchronize()
    assert W.last_kernel.startswith("team2r<4")
    want1, want2 = C1.clone(), C2.clone()
    A = hip.CsrDev(M, K, ctx.rp, ctx.ci, ctx.va)
    ctx.keep.append(A)
    ops.poison()
    ops.clear()
    C2.fill_(H.SENTINEL)
    torch.cuda.synchronize()
    S2 = held.second()
    with torch.cuda.stream(held.S):
        held.hold()
        ops.load(0)
        ops.clear()
        hip.spmm_csr(A, B, C1, variant=7)
    with torch.cuda.stream(S2):
        hip.spmm_csr(A, B2, C2, variant=7)
    S2.synchronize()
    held.S.synchronize()
    torch.cuda.synchronize()
    assert H.same([C2], [want2]) and H.same([C1], [want1])


# ---- part B: the engines on a caller's stream (world 1, timing off) ----------------------------------------------------------

EN = 24                              # the engines' width


class Engines:
    def __init__(self, c):
        from crp_spmm_amd import comm, engine, gen
        self.c = c
        self.sc = [comm.SelfComm() for _ in range(2)]
        self.rp = engine.RpSpmm(0, M, c.rp, c.ci, c.va, [0, K], EN, self.sc[0])
        self.sq = gen.random_csr(M, M, 30, seed=5, empty_every=13)
        self.p2 = engine.Para2dSpmm(self.sc[1], 1, 1, [0, M], [0, M], [0, M], [0, EN], *self.sq)
        self.rp.set_timing(False)
        self.p2.rp.set_timing(False)

    def close(self):
        self.rp.free()
        self.p2.free()
        for s in self.sc:
            s.free()


@pytest.fixture(scope="module")
def engines(ctx):
    e = Engines(ctx)
    yield e
    e.close()


def _engine_rows():
    """(id, which engine, blocking, builder(engine, nnz, ncol, ops) -> call)"""
    import torch

    def exec_(dt):
        return lambda e, nnz, k, ops: (lambda B, C: (lambda stream: e.exec(0, B, C, stream=stream)))(ops.dense(_rnd(51, (k, EN), dt)), ops.out((M, EN), _tdt(dt)))

    def exec_t(dt):
        def b(e, nnz, k, ops):
            B, C = ops.dense(_rnd(52, (M, EN), dt)), ops.out((k, EN), _tdt(dt))
            fn = e.exec_t if np.dtype(dt) == np.float64 else e.exec_t_f32
            return lambda stream: fn(0, B, C, stream=stream)
        return b

    def sddmm(dt, mode):
        def b(e, nnz, k, ops):
            X, Y, out = ops.dense(_rnd(53, (M, EN), dt)), ops.dense(_rnd(54, (k, EN), dt)), ops.out((nnz,), _tdt(dt))
            return lambda stream: e.sddmm(0, X, Y, out, mode=mode, stream=stream)
        return b

    def softmax(dt, bwd):
        def b(e, nnz, k, ops):
            s, out = ops.dense(_rnd(55, (nnz,), dt)), ops.out((nnz,), _tdt(dt))
            if not bwd:
                return lambda stream: e.row_softmax(s, out=out, stream=stream)
            dy = ops.dense(_rnd(56, (nnz,), dt))
            return lambda stream: e.row_softmax_bwd(s, dy, out=out, stream=stream)
        return b

    def attention(dt):
        def b(e, nnz, k, ops):
            Q, Kk, V = (ops.dense(_rnd(57 + i, sh, dt)) for i, sh in enumerate(((M, EN), (k, EN), (k, EN))))
            O, lse, p = ops.out((M, EN), _tdt(dt)), ops.out((M,), _tdt(dt)), ops.out((nnz,), _tdt(dt))
            return lambda stream: e.attention(0, Q, Kk, V, O, scale=0.2, bias=True, lse=lse, p_out=p, stream=stream)
        return b

    def attention_bwd(dt):
        def b(e, nnz, k, ops):
            t = [torch.from_numpy(_rnd(60 + i, sh, dt)).to(ops.gpu) for i, sh in enumerate(((M, EN), (k, EN), (k, EN), (M, EN)))]
            d = []
            for sgn in (1.0, -0.5):                               # two consistent data sets: O and lse from the engine's forward
                Q, Kk, V, dO = (x * sgn for x in t)
                O, lse = torch.empty((M, EN), dtype=Q.dtype, device=ops.gpu), torch.empty((M,), dtype=Q.dtype, device=ops.gpu)
                e.attention(0, Q, Kk, V, O, scale=0.2, bias=True, lse=lse)
                torch.cuda.synchronize()
                d.append((Q, Kk, V, O, dO, lse))
            Q, Kk, V, O, dO, lse = (ops.dense(a, b_) for a, b_ in zip(*d))
            dQ, dK, dV, ds = (ops.out(sh, _tdt(dt)) for sh in ((M, EN), (k, EN), (k, EN), (nnz,)))
            return lambda stream: e.attention_bwd(Q, Kk, V, O, dO, lse, dQ, dK, dV, scale=0.2, bias=True, ds_out=ds, stream=stream)
        return b

    def update_dev(dt):
        def b(e, nnz, k, ops):
            vals = ops.dense(np.random.default_rng(61).uniform(-2, 2, nnz).astype(dt))
            B, C = ops.dense(_rnd(62, (k, EN))), ops.out((M, EN), torch.float64)

            def call(stream):
                e.update_values_dev(vals, stream=stream)
                e.exec(0, B, C, stream=stream)
            return call
        return b

    rows = []
    for eng in ("rp", "para2d"):
        rows += [("%s-exec-%s" % (eng, np.dtype(dt).name), eng, None, exec_(dt)) for dt in (F64, F32)]
        rows += [("%s-exec_t" % eng, eng, None, exec_t(F64)), ("%s-exec_t_f32" % eng, eng, None, exec_t(F32))]
        rows += [("%s-sddmm-%s-mode%d" % (eng, np.dtype(dt).name, mode), eng, None, sddmm(dt, mode)) for dt in (F64, F32) for mode in (0, 1)]
        rows += [("%s-row_softmax%s-%s" % (eng, "_bwd" if bwd else "", np.dtype(dt).name), eng, None, softmax(dt, bwd))
                 for bwd in (False, True) for dt in (F64, F32)]
        rows += [("%s-update_values_dev-%s-then-exec" % (eng, np.dtype(dt).name), eng, None, update_dev(dt)) for dt in (F64, F32)]
    rows += [("rp-attention-%s" % np.dtype(dt).name, "rp", None, attention(dt)) for dt in (F64, F32)]
    rows += [("rp-attention_bwd-%s" % np.dtype(dt).name, "rp", None, attention_bwd(dt)) for dt in (F64, F32)]
    rows += [("rp-exec-timing-on", "rp", "timing-on", exec_(F64))]
    return rows


ENGINE_ROWS = _engine_rows()


@pytest.mark.parametrize("name,which,blocking,build", ENGINE_ROWS, ids=[r[0] for r in ENGINE_ROWS])
def test_engine_order_asynchrony_control(ctx, engines, name, which, blocking, build):
    e = engines.rp if which == "rp" else engines.p2
    nnz, k = (ctx.ci.size, K) if which == "rp" else (engines.sq[1].size, M)
    ops = H.Operands(ctx.gpu)
    call = build(e, nnz, k, ops)
    held = ctx.held
    timed = e if which == "rp" else e.rp
    timed.set_timing(blocking == "timing-on")
    try:
        want = held.reference(ops, call, name=None if blocking else name)
        held.warm(ops, call)
        got, pending = held.run(ops, call)
        assert H.same(got, want), "Order"
        if not blocking:
            assert pending, "Asynchrony"
        bad, _ = held.run(ops, call, stream=0)
        held.heal(ops, call)
        assert not H.same(bad, want), "Control"
    finally:
        timed.set_timing(False)


def _exec(e, B, k=K):
    """the engine's product of B on the current stream -> C"""
    import torch
    C = torch.full((M, EN), H.SENTINEL, dtype=torch.float64, device=B.device)
    e.exec(0, B, C)
    return C


@pytest.fixture()
def rp_engine(ctx):
    """a row-parallel engine of its own (the ordering cases change its values), timing off, with its three value sets and the
    product each gives on the default stream"""
    import torch
    from crp_spmm_amd import comm, engine
    sc = comm.SelfComm()
    e = engine.RpSpmm(0, M, ctx.rp, ctx.ci, ctx.va, [0, K], EN, sc)
    e.set_timing(False)
    B = torch.from_numpy(_rnd(71, (K, EN))).to(ctx.gpu)
    vals = [ctx.va, np.random.default_rng(72).uniform(-2, 2, ctx.ci.size), np.random.default_rng(73).uniform(-2, 2, ctx.ci.size)]
    want = []
    for v in vals:
        e.update_values(v)
        want.append(_exec(e, B))
        torch.cuda.synchronize()
    e.update_values(vals[0])
    dev = [torch.from_numpy(v).to(ctx.gpu) for v in vals]
    e.update_values_dev(dev[0])                                   # (the first device update allocates its scratch: it blocks once)
    torch.cuda.synchronize()
    assert H.same([_exec(e, B)], [want[0]])
    torch.cuda.synchronize()
    yield e, B, dev, vals, want
    torch.cuda.synchronize()
    e.free()
    sc.free()


def test_engine_update_does_not_overtake_an_exec(ctx, rp_engine):
    """exec on the held-back S, then update_values_dev(new) on the free S2 with no caller ordering: C is the product with the OLD
    values (the update waits for ev_exec), and a following exec on S2 gives the new ones"""
    import torch
    e, B, dev, vals, want = rp_engine
    held = ctx.held
    S2 = held.second()
    ops = H.Operands(ctx.gpu)
    Bl = ops.dense(B)
    C = ops.out((M, EN), torch.float64)
    ops.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(held.S):
        held.hold()
        ops.load(0)
        ops.clear()
        e.exec(0, Bl, C)
    with torch.cuda.stream(S2):
        e.update_values_dev(dev[1])
        C2 = _exec(e, B)
    S2.synchronize()
    held.S.synchronize()
    torch.cuda.synchronize()
    assert H.same([C], [want[0]]), "the value update overtook the exec in flight on the other stream"
    assert H.same([C2], [want[1]])


def test_engine_two_device_updates_on_two_streams(ctx, rp_engine):
    """update_values_dev(v1) on the held-back S, then update_values_dev(v2) on the free S2: the engine holds v2 (ev_vals)"""
    import torch
    e, B, dev, vals, want = rp_engine
    held = ctx.held
    S2 = held.second()
    ops = H.Operands(ctx.gpu)
    v1 = ops.dense(dev[1])
    ops.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(held.S):
        held.hold()
        ops.load(0)
        e.update_values_dev(v1)
    with torch.cuda.stream(S2):
        e.update_values_dev(dev[2])
    S2.synchronize()
    held.S.synchronize()
    torch.cuda.synchronize()
    assert H.same([_exec(e, B)], [want[2]]), "the later update did not wait for the earlier one on the other stream"


def test_engine_device_update_before_a_host_update(ctx, rp_engine):
    """update_values_dev(v1) on the held-back S, then the host update_values(v2), which runs on the engine's own stream: the
    engine holds v2 (its stream waits for ev_vals)"""
    import torch
    e, B, dev, vals, want = rp_engine
    held = ctx.held
    ops = H.Operands(ctx.gpu)
    v1 = ops.dense(dev[1])
    ops.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(held.S):
        held.hold()
        ops.load(0)
        e.update_values_dev(v1)
    e.update_values(vals[2])
    held.S.synchronize()
    torch.cuda.synchronize()
    assert H.same([_exec(e, B)], [want[2]]), "the host update did not wait for the device update on the caller's stream"


def test_engine_first_attention_bwd_after_a_held_back_device_update(ctx):
    """update_values_dev(v1) on the held-back S, then the FIRST attention_bwd with bias: it builds the transposed matrices from
    the device values it downloads on the engine's own stream, which waits for the update.  Equal to the handle-level calls with
    v1, bit for bit."""
    import torch
    from crp_spmm_amd import comm, engine, hip
    held = ctx.held
    gpu = ctx.gpu
    v1 = np.random.default_rng(81).uniform(-2, 2, ctx.ci.size)
    A, At = hip.CsrDev(M, K, ctx.rp, ctx.ci, v1), hip.CsrDev.from_transpose(M, K, ctx.rp, ctx.ci, v1)
    ctx.keep += [A, At]
    Q, Kk, V, dO = (torch.from_numpy(_rnd(82 + i, sh)).to(gpu) for i, sh in enumerate(((M, EN), (K, EN), (K, EN), (M, EN))))
    lse = torch.empty((M,), dtype=torch.float64, device=gpu)
    O = A.attention(Q, Kk, V, scale=0.2, bias=True, lse=lse)
    ds = torch.empty((A.nnz,), dtype=torch.float64, device=gpu)
    dQ, delta = A.attention_bwd_q(Q, Kk, V, O, dO, lse, scale=0.2, bias=True, ds_out=ds)
    dK, dV = At.attention_bwd_kv(Kk, V, Q, dO, lse, delta, scale=0.2, bias=True)
    torch.cuda.synchronize()
    want = [dQ, dK, dV, ds]
    sc = comm.SelfComm()
    e = engine.RpSpmm(0, M, ctx.rp, ctx.ci, ctx.va, [0, K], EN, sc)
    e.set_timing(False)
    try:
        warm = torch.from_numpy(ctx.va).to(gpu)
        e.update_values_dev(warm)                                 # (allocates the update's scratch; the values stay)
        torch.cuda.synchronize()
        assert not e.transposed_built and not e.attention_bwd_built()
        ops = H.Operands(gpu)
        vals = ops.dense(v1)
        outs = [ops.out(sh, torch.float64) for sh in ((M, EN), (K, EN), (K, EN), (A.nnz,))]
        ops.poison()
        torch.cuda.synchronize()
        with torch.cuda.stream(held.S):
            held.hold()
            ops.load(0)
            ops.clear()
            e.update_values_dev(vals)
            e.attention_bwd(Q, Kk, V, O, dO, lse, *outs[:3], scale=0.2, bias=True, ds_out=outs[3])
            got = ops.snapshot()
        held.S.synchronize()
        torch.cuda.synchronize()
        assert e.transposed_built
        assert H.same(got, want), "the transposed matrices were built from values the update had not written yet"
    finally:
        torch.cuda.synchronize()
        e.free()
        sc.free()


def test_the_delay_covers_the_slowest_host_call(ctx):
    """after every row above (same module, same Ctx): the calibrated delay is at least 100 times the slowest steady-state host
    call timed in this run on the default stream, and at most 250 ms"""
    held = ctx.held
    if not held.host_ms:
        for name, blocking, build in TABLE:
            if blocking is None:
                ops, call = build(ctx)
                held.reference(ops, call, name=name)
    held.calibrate()
    slow = max(held.host_ms, key=held.host_ms.get)
    print("slowest steady-state host call: %s %.3f ms; delay %.1f ms (%.4g cycles per ms)"
          % (slow, held.host_ms[slow], held.delay_ms, held.cycles_per_ms))
    assert held.delay_ms >= 100 * held.host_ms[slow], (slow, held.host_ms[slow], held.delay_ms)
    assert held.delay_ms <= H.DELAY_MAX_MS


def test_engines_on_a_side_stream_world_2():
    """tests/gpu_dist_streams_worker.py: every engine call on a side stream, two ranks sharing the GPU, host-staged exchange"""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    env.pop("CRPSPMM_EXPECT_NATIVE_RCCL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "gpu_dist_streams_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_STREAMS_WORKER_OK world=2" in r.stdout
