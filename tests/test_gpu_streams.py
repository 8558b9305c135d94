"""GPU: the stream contract of include/crpspmm_hip.h ("Streams") and include/crp_engine.h, on a held-back non-blocking side
stream (tests/streams_harness.py, which explains the method).  Measured on the MI355X: the slowest steady-state host call of the
table is hip.gatv2_attention forward + backward with dropout at 0.39 ms (the least of three), the delay is 120 ms (2.39e6 cycles
of torch.cuda._sleep per ms).

What the rows must reach is read from the headers, not kept by hand: every crp_* prototype of include/crpspmm_hip.h and
include/crp_engine.h with a `void *stream` parameter (stream_entry_points) that is not in EXEMPT -- plumbing and probes, each
with its reason -- is really called by the reference call of a row of TABLE or ENGINE_ROWS, which is observed on the loaded
library object (test_every_stream_taking_entry_point_is_reached); an entry point added to a header without a row fails it.
TABLE also names every product launcher (test_the_table_reaches_every_launcher), each on the smallest matrix that reaches it; the
kernels' numerics are pinned elsewhere.  Every row makes three assertions -- Order, Asynchrony, Control -- and every row that is not `blocking` is also
captured into a graph on the side stream and replayed on a second data set.

Order is asserted BIT FOR BIT in every row: the header promises repeatability for every call of the table (crp_spmm_csr_f64:
"repeated calls are bit-identical"; crp_sddmm_csr_*, the row softmax, crp_scatter_add_rows_*, crp_sum_segments_*: "Repeated calls
are ... bit-identical"; the attention calls and their backward: "A row's bits depend on (dtype, nk, nv, scale, bias) and the row's
entries in CSR order ONLY"; the GAT and GATv2 calls: "O, lse and p_out are bit for bit what that order gives", every backward sum
"from +0 in ascending p" or in the handle's CSR order; their _drop_ forms and crp_dropout_mask_csr: "the keep bit of an edge is a
pure function of (seed, r, c, h)"; crp_col_sum_*: "repeated calls are bit-identical"; the fp32 products are pinned exactly by
tests/test_gpu_fp32_kernels.py; the row movers only move), so no row falls back to a bound.

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
    "other-heads": "that call blocks, as does a call with another number of heads, which sets them up again",
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


# ---- completeness: the stream-taking entry points are read from the headers, not kept by hand -------------------------------

# entry points that take a stream and launch no compute kernel: plumbing and probes.  Everything else must be reached by a row.
EXEMPT = {
    "crp_dev_memset": "plumbing: hipMemsetAsync on the stream it is given",
    "crp_dev_memcpy": "plumbing: hipMemcpyAsync on the stream it is given",
    "crp_dev_memcpy2d": "plumbing: hipMemcpy2DAsync on the stream it is given",
    "crp_stream_destroy": "plumbing: the stream is the object, not where work goes",
    "crp_stream_sync": "plumbing: the stream is the object, not where work goes",
    "crp_stream_wait_event": "plumbing: the stream is the object, not where work goes",
    "crp_event_record": "plumbing: hipEventRecord on the stream it is given",
    "crp_probe_stamp": "probe: a one-thread kernel that writes the device clock, a diagnostic of tools/overlap_probe.py",
    "crp_probe_copy": "probe: a stand-in for a transport's copy kernel with clock stamps, a diagnostic of tools/overlap_probe.py",
}
_EXEMPT_KIND = re.compile(r"crp_(dev_mem(set|cpy|cpy2d)|stream_\w+|event_record|probe_\w+)$")


def stream_entry_points(header):
    """every crp_* prototype of include/<header> with a `void *stream` parameter, comments stripped first"""
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    return {m.group(1) for m in re.finditer(r"\b(crp_\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))}


def test_the_headers_name_their_stream_taking_entry_points():
    """the parse finds something, old and new: a regular expression that silently matches nothing fails here.  (The counts are the
    headers' of today; a new entry point changes them, and test_every_stream_taking_entry_point_is_reached then asks for its row.)"""
    dev, eng = stream_entry_points("crpspmm_hip.h"), stream_entry_points("crp_engine.h")
    assert {"crp_spmm_csr_f64", "crp_csr_dev_update_values", "crp_gatv2_attention_drop_bwd_col_csr_f32", "crp_dropout_mask_csr",
            "crp_col_sum_f32"} <= dev, sorted(dev)
    assert {"crp_rp_spmm_exec_ex", "crp_para2d_spmm_update_values_dev", "crp_rp_spmm_gatv2_f32_ex", "crp_rp_spmm_attention_bwd_mh_ex"} <= eng, sorted(eng)
    assert len(dev) >= 74 and len(eng) >= 30, (len(dev), len(eng))
    assert not dev & eng
    assert set(EXEMPT) <= dev and all(_EXEMPT_KIND.match(name) for name in EXEMPT), sorted(set(EXEMPT) - dev)
    assert "crp_stream_create" not in dev                      # (takes a void **: where the stream is made, not used)


class _observed:
    """While a call runs, every stream-taking entry point of the loaded library object is wrapped: the names that are REALLY
    called are added to `reached`.  The wrappers are attributes of the library object, which is where the Python layer looks an
    entry point up for every call; the originals are put back on exit."""

    def __init__(self, lib, reached):
        self.lib, self.reached, self.saved = lib, reached, {}

    def __enter__(self):
        names = (stream_entry_points("crpspmm_hip.h") | stream_entry_points("crp_engine.h")) - set(EXEMPT)
        for name in names:
            fn = getattr(self.lib, name)

            def spy(*args, _fn=fn, _name=name):
                self.reached.add(_name)
                return _fn(*args)
            spy.__name__ = name
            self.saved[name] = fn
            setattr(self.lib, name, spy)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)
        return False


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
        self.cache_data = {}                 # staging data that takes a forward to make (_gat_data), made once
        self.reached = set()                 # the stream-taking entry points the rows' reference calls went through (_observed)

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


def _attn_data(c, dt, seed, nk=16, nv=24, heads=1):
    """Q, K, V, dO and what the forward writes for them on the default stream: O, lse (staging data of the backward rows); with
    `heads` > 1 that many heads of nk / nv columns side by side, lse and delta (rows, heads)"""
    import torch
    import attention_bwd_ref as B
    A = c.handle("B")
    nk, nv = nk * heads, nv * heads
    Q, Kk, V, dO = (torch.from_numpy(_rnd(seed + i, sh, dt)).to(c.gpu)
                    for i, sh in enumerate(((B.NROW, nk), (B.NCOL, nk), (B.NCOL, nv), (B.NROW, nv))))
    lse = torch.empty((B.NROW,) if heads == 1 else (B.NROW, heads), dtype=Q.dtype, device=c.gpu)
    O = A.attention(Q, Kk, V, scale=0.25, bias=True, lse=lse, heads=heads)
    dQ, delta = A.attention_bwd_q(Q, Kk, V, O, dO, lse, scale=0.25, bias=True, heads=heads)
    torch.cuda.synchronize()
    return dict(Q=Q, K=Kk, V=V, dO=dO, O=O, lse=lse, delta=delta)


def _per_head(count, heads):
    """the shape of a per-row or per-nonzero vector: 1-D with one head, (count, heads) with several"""
    return (count,) if heads == 1 else (count, heads)


def _attention(dt, heads=1):
    def build(c):
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        A = c.handle("B")
        d0, d1 = _attn_data(c, dt, 10, heads=heads), _attn_data(c, dt, 20, heads=heads)
        Q, Kk, V = (ops.dense(d0[k], d1[k]) for k in ("Q", "K", "V"))
        O, lse, p = (ops.out(sh, _tdt(dt)) for sh in ((B.NROW, 24 * heads), _per_head(B.NROW, heads), _per_head(A.nnz, heads)))
        return ops, lambda stream: A.attention(Q, Kk, V, scale=0.25, bias=True, out=O, lse=lse, p_out=p, stream=stream, heads=heads)
    return build


def _attention_bwd_q(dt, heads=1):
    def build(c):
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        A = c.handle("B")
        d0, d1 = _attn_data(c, dt, 10, heads=heads), _attn_data(c, dt, 20, heads=heads)
        Q, Kk, V, O, dO, lse = (ops.dense(d0[k], d1[k]) for k in ("Q", "K", "V", "O", "dO", "lse"))
        dQ, delta, ds = (ops.out(sh, _tdt(dt)) for sh in ((B.NROW, 16 * heads), _per_head(B.NROW, heads), _per_head(A.nnz, heads)))
        return ops, lambda stream: A.attention_bwd_q(Q, Kk, V, O, dO, lse, scale=0.25, bias=True, dQ=dQ, delta=delta, ds_out=ds,
                                                     stream=stream, heads=heads)
    return build


def _attention_bwd_kv(dt, in_place=False, heads=1):
    def build(c):
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        At = c.handle("Bt")
        d0, d1 = _attn_data(c, dt, 10, heads=heads), _attn_data(c, dt, 20, heads=heads)
        Kk, V = (ops.dense(d0[k], d1[k], inout=in_place) for k in ("K", "V"))
        Q, dO, lse, delta = (ops.dense(d0[k], d1[k]) for k in ("Q", "dO", "lse", "delta"))
        dK, dV = (Kk, V) if in_place else (ops.out((B.NCOL, 16 * heads), _tdt(dt)), ops.out((B.NCOL, 24 * heads), _tdt(dt)))
        return ops, lambda stream: At.attention_bwd_kv(Kk, V, Q, dO, lse, delta, scale=0.25, bias=True, dK=dK, dV=dV, stream=stream,
                                                       heads=heads)
    return build


HEADS, DV, SLOPE, SEED = 2, 12, 0.2, 0x5EED5EED12345         # the GAT / GATv2 rows: two heads of 12 columns


def _gat_data(c, dt, seed, v2, dropout):
    """The operands of the GAT (v2: GATv2) rows on the handles "B" / "Bt" and what a real forward and row-side backward write for
    them on the default stream -- O, lse, delta: staging data of the backward rows, which need them consistent.  Made once."""
    import torch
    import attention_bwd_ref as B
    key = ("gat-data", np.dtype(dt).name, seed, v2, dropout)
    if key in c.cache_data:
        return c.cache_data[key]
    A = c.handle("B")
    n = HEADS * DV
    kw = dict(slope=SLOPE, bias=True, heads=HEADS, dropout=dropout, seed=SEED)
    lse = torch.empty((B.NROW, HEADS), dtype=_tdt(dt), device=c.gpu)
    T = lambda i, sh: torch.from_numpy(_rnd(seed + i, sh, dt)).to(c.gpu)
    dO = T(0, (B.NROW, n))
    if v2:
        d = dict(XT=T(1, (B.NROW, n)), XS=T(2, (B.NCOL, n)), a=T(3, (HEADS, DV)), dO=dO, lse=lse)
        d["O"] = A.gatv2_attention(d["XT"], d["XS"], d["a"], lse=lse, **kw)
        _, d["da_part"], d["delta"] = A.gatv2_attention_bwd_row(d["XT"], d["XS"], d["a"], d["O"], dO, lse, **kw)
    else:
        d = dict(el=T(1, (B.NROW, HEADS)), er=T(2, (B.NCOL, HEADS)), V=T(3, (B.NCOL, n)), dO=dO, lse=lse)
        d["O"] = A.gat_attention(d["el"], d["er"], d["V"], lse=lse, **kw)
        _, d["delta"] = A.gat_attention_bwd_row(d["el"], d["er"], d["V"], d["O"], dO, lse, **kw)
    torch.cuda.synchronize()
    c.cache_data[key] = d
    return d


def _gat(dt, what, dropout, v2=False):
    """gat_attention / gatv2_attention (what "fwd"), their row side with ds_out ("bwd_row") and their column side ("bwd_col");
    dropout 0 reaches the plain entry points, dropout > 0 the _drop_ ones"""
    def build(c):
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        A, At = c.handle("B"), c.handle("Bt")
        d0, d1 = _gat_data(c, dt, 100, v2, dropout), _gat_data(c, dt, 200, v2, dropout)
        n, t = HEADS * DV, _tdt(dt)
        kw = dict(slope=SLOPE, bias=True, heads=HEADS, dropout=dropout, seed=SEED)
        D = lambda *names: tuple(ops.dense(d0[k], d1[k]) for k in names)
        if what == "fwd":
            x = D("XT", "XS", "a") if v2 else D("el", "er", "V")
            O, lse, p = ops.out((B.NROW, n), t), ops.out((B.NROW, HEADS), t), ops.out((A.nnz, HEADS), t)
            fn = A.gatv2_attention if v2 else A.gat_attention
            return ops, lambda stream: fn(*x, out=O, lse=lse, p_out=p, stream=stream, **kw)
        if what == "bwd_row":
            x = D("XT", "XS", "a", "O", "dO", "lse") if v2 else D("el", "er", "V", "O", "dO", "lse")
            delta, ds = ops.out((B.NROW, HEADS), t), ops.out((A.nnz, HEADS), t)
            if v2:
                dXT, da_part = ops.out((B.NROW, n), t), ops.out((B.NROW, n), t)
                return ops, lambda stream: A.gatv2_attention_bwd_row(*x, dXT=dXT, da_part=da_part, delta=delta, ds_out=ds, stream=stream, **kw)
            d_el = ops.out((B.NROW, HEADS), t)
            return ops, lambda stream: A.gat_attention_bwd_row(*x, d_el=d_el, delta=delta, ds_out=ds, stream=stream, **kw)
        if v2:
            x = D("XS", "XT", "a", "dO", "lse", "delta")
            dXS = ops.out((B.NCOL, n), t)
            return ops, lambda stream: At.gatv2_attention_bwd_col(*x, dXS=dXS, stream=stream, **kw)
        x = D("er", "V", "el", "dO", "lse", "delta")
        d_er, dV = ops.out((B.NCOL, HEADS), t), ops.out((B.NCOL, n), t)
        return ops, lambda stream: At.gat_attention_bwd_col(*x, d_er=d_er, dV=dV, stream=stream, **kw)
    return build


def _gat_two_source(v2):
    """the forward on the two-source handle: er1 / V1 (v2: XS1) are the rows the negative column codes name; p_out through out_pos"""
    def build(c):
        import torch
        ops = H.Operands(c.gpu)
        A = c.handle("A2")
        n, t = HEADS * DV, torch.float64
        pos = torch.from_numpy(np.random.default_rng(6).permutation(A.nnz).astype(np.int32)).to(c.gpu)
        O, lse, p = ops.out((M, n), t), ops.out((M, HEADS), t), ops.out((A.nnz, HEADS), t)
        kw = dict(slope=SLOPE, bias=True, heads=HEADS, out=O, lse=lse, p_out=p, out_pos=pos)
        if v2:
            XT, XS0, XS1, a = (ops.dense(_rnd(110 + i, sh)) for i, sh in enumerate(((M, n), (HALF, n), (K - HALF, n), (HEADS, DV))))
            return ops, lambda stream: A.gatv2_attention(XT, XS0, a, XS1=XS1, stream=stream, **kw)
        el, er0, er1, V0, V1 = (ops.dense(_rnd(120 + i, sh)) for i, sh in
                                enumerate(((M, HEADS), (HALF, HEADS), (K - HALF, HEADS), (HALF, n), (K - HALF, n))))
        return ops, lambda stream: A.gat_attention(el, er0, V0, er1=er1, V1=V1, stream=stream, **kw)
    return build


def _col_sum(dt):
    """hip.col_sum on an operand shaped like da_part of the GATv2 row side (its scratch comes from torch's allocator)"""
    def build(c):
        from crp_spmm_amd import hip
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        d0, d1 = _gat_data(c, dt, 100, True, 0.0), _gat_data(c, dt, 200, True, 0.0)
        src, out = ops.dense(d0["da_part"], d1["da_part"]), ops.out((HEADS * DV,), _tdt(dt))
        assert tuple(src.shape) == (B.NROW, HEADS * DV)
        return ops, lambda stream: hip.col_sum(src, out=out, stream=stream)
    return build


def _dropout_mask(c):
    """dropout_mask has no dense value input: its one operand is the output, whose sentinel fill (int8 -77, handed over as the
    uint8 view the wrapper takes) lies on the held-back stream, behind a launch that went elsewhere"""
    import torch
    ops = H.Operands(c.gpu)
    A = c.handle("B")
    out = ops.out((A.nnz, HEADS), torch.int8)
    return ops, lambda stream: A.dropout_mask(HEADS, 0.25, SEED, out=out.view(torch.uint8), stream=stream)


def _gat_autograd(v2, dropout):
    """hip.gat_attention / hip.gatv2_attention forward and .backward (v2: with col_sum): no stream argument anywhere, the control
    makes the null stream current"""
    def build(c):
        import torch
        from crp_spmm_amd import hip
        import attention_bwd_ref as B
        ops = H.Operands(c.gpu)
        A, At = c.handle("B"), c.handle("Bt")
        d0, d1 = _gat_data(c, F64, 100, v2, dropout), _gat_data(c, F64, 200, v2, dropout)
        n = HEADS * DV
        names = ("XT", "XS", "a") if v2 else ("el", "er", "V")
        x = tuple(ops.dense(d0[k], d1[k]) for k in names)
        dO = ops.dense(d0["dO"], d1["dO"])
        outs = [ops.out(sh, torch.float64) for sh in ((B.NROW, n),) + tuple(tuple(t.shape) for t in x)]
        fn = hip.gatv2_attention if v2 else hip.gat_attention

        def run():
            leaves = tuple(t.detach().requires_grad_(True) for t in x)
            O = fn(A, At, *leaves, slope=SLOPE, bias=True, heads=HEADS, dropout=dropout, seed=SEED)
            grads = torch.autograd.grad(O, leaves, dO)
            for dst, src in zip(outs, (O.detach(),) + tuple(grads)):
                dst.copy_(src)

        def call(stream):
            if stream is None:
                return run()
            with torch.cuda.stream(torch.cuda.default_stream()):
                run()
        return ops, call
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
    """the device helpers without a Python wrapper: the raw library call on torch's current stream (the entry point is looked up
    on the library object at every call, as the wrappers do)"""
    def build(c):
        import torch
        from crp_spmm_amd import _lib as L
        ops = H.Operands(c.gpu)
        raw = lambda name, *args: L.check(getattr(c.lib, name)(*args), name)
        sfx = "f32" if np.dtype(dt) == np.float32 else "f64"
        if what == "scatter_add_rows":
            n, nseg, nsrc = 9, 40, 100
            rng = np.random.default_rng(14)
            seg_row = torch.from_numpy(rng.permutation(64)[:nseg].astype(np.int32)).to(c.gpu)              # distinct rows
            cnt = rng.integers(0, 5, nseg)
            seg_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)).to(c.gpu)
            seg_pos = torch.from_numpy(rng.integers(0, nsrc, int(cnt.sum())).astype(np.int32)).to(c.gpu)
            src, dst = ops.dense(_rnd(15, (nsrc, n), dt)), ops.dense(_rnd(16, (64, n), dt), inout=True)
            return ops, lambda stream: raw("crp_scatter_add_rows_" + sfx, nseg, n, seg_row.data_ptr(), seg_ptr.data_ptr(), seg_pos.data_ptr(),
                                           src.data_ptr(), n, dst.data_ptr(), n, _cur(stream))
        if what == "gather_vals":
            cnt = 700
            vmap = torch.from_numpy(np.random.default_rng(17).integers(0, 500, cnt).astype(np.int32)).to(c.gpu)
            src, dst = ops.dense(_rnd(18, (500,), dt)), ops.out((cnt,), torch.float64)
            name = "crp_gather_vals_f32_f64" if sfx == "f32" else "crp_gather_vals_f64"
            return ops, lambda stream: raw(name, cnt, vmap.data_ptr(), src.data_ptr(), dst.data_ptr(), _cur(stream))
        nseg, ln = 3, 259
        src, out = ops.dense(_rnd(19, (nseg * ln,), dt)), ops.out((ln,), _tdt(dt))
        return ops, lambda stream: raw("crp_sum_segments_" + sfx, nseg, ln, src.data_ptr(), ln, out.data_ptr(), _cur(stream))
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
_DT = [(F64, "float64"), (F32, "float32")]
TABLE += [("attention-heads2-%s" % nm, None, _attention(dt, heads=HEADS)) for dt, nm in _DT]
TABLE += [("attention_bwd_q-heads2-%s" % nm, None, _attention_bwd_q(dt, heads=HEADS)) for dt, nm in _DT]
TABLE += [("attention_bwd_kv-heads2-%s" % nm, None, _attention_bwd_kv(dt, heads=HEADS)) for dt, nm in _DT]
TABLE += [("attention_bwd_kv-heads2-in-place-%s" % nm, None, _attention_bwd_kv(dt, in_place=True, heads=HEADS)) for dt, nm in _DT]
for _v2, _fam in ((False, "gat_attention"), (True, "gatv2_attention")):
    TABLE += [("%s%s-%s%s" % (_fam, {"fwd": ""}.get(what, "_" + what), nm, "-dropout" if drop else ""), None, _gat(dt, what, drop, v2=_v2))
              for what in ("fwd", "bwd_row", "bwd_col") for dt, nm in _DT for drop in (0.0, 0.25)]
    TABLE += [("%s-two-source" % _fam, None, _gat_two_source(_v2))]
TABLE += [("col_sum-%s" % nm, None, _col_sum(dt)) for dt, nm in _DT]
TABLE += [("dropout_mask", None, _dropout_mask)]
TABLE += [("hip.%s-forward-backward%s" % (_fam, "-dropout" if drop else ""), None, _gat_autograd(_v2, drop))
          for _v2, _fam in ((False, "gat_attention"), (True, "gatv2_attention")) for drop in (0.0, 0.25)]
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
    with _observed(ctx.lib, ctx.reached):
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


def test_first_fp32_gat_attention_on_one_stream_then_a_product_on_another(ctx):
    """The same case with the fp32 copy of the values built by the first fp32 gat_attention with bias, on a fresh handle on the
    held-back S1; then an independent fp32 product of the same handle on the free S2, nothing ordering the two: both are correct."""
    import torch
    from crp_spmm_amd import hip
    import attention_bwd_ref as B
    n = HEADS * DV
    held = ctx.held
    rp, ci, nrow = B.matrix()
    va = np.random.default_rng(3).uniform(-1, 1, ci.size)
    ops = H.Operands(ctx.gpu)
    el, er, V = (ops.dense(_rnd(34 + i, sh, np.float32)) for i, sh in enumerate(((nrow, HEADS), (B.NCOL, HEADS), (B.NCOL, n))))
    O, lse = ops.out((nrow, n), torch.float32), ops.out((nrow, HEADS), torch.float32)
    B2 = torch.from_numpy(_rnd(37, (B.NCOL, n), np.float32)).to(ctx.gpu)
    C2 = torch.full((nrow, n), H.SENTINEL, dtype=torch.float32, device=ctx.gpu)
    gat = lambda h: h.gat_attention(el, er, V, slope=SLOPE, bias=True, out=O, lse=lse, heads=HEADS)
    W = hip.CsrDev(nrow, B.NCOL, rp, ci, va)                      # the reference: a handle of its own, on the default stream
    ctx.keep.append(W)
    ops.load(0)
    gat(W)
    hip.spmm_csr_f32(W, B2, C2, variant=1)
    torch.cuda.synchronize()
    assert W.last_kernel.startswith("rowgroup_f32<")
    want1, want2 = ops.snapshot(), C2.clone()
    A = hip.CsrDev(nrow, B.NCOL, rp, ci, va)
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
        gat(A)
    with torch.cuda.stream(S2):
        hip.spmm_csr_f32(A, B2, C2, variant=1)
    S2.synchronize()
    held.S.synchronize()
    torch.cuda.synchronize()
    assert H.same([C2], [want2]), "the product on the second stream read values the first gat_attention had not finished converting"
    assert H.same(ops.snapshot(), want1)


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

    def attention(dt, heads=1):
        def b(e, nnz, k, ops):
            Q, Kk, V = (ops.dense(_rnd(57 + i, sh, dt)) for i, sh in enumerate(((M, EN), (k, EN), (k, EN))))
            O, lse, p = ops.out((M, EN), _tdt(dt)), ops.out(_per_head(M, heads), _tdt(dt)), ops.out(_per_head(nnz, heads), _tdt(dt))
            return lambda stream: e.attention(0, Q, Kk, V, O, scale=0.2, bias=True, lse=lse, p_out=p, stream=stream, heads=heads)
        return b

    def attention_bwd(dt, heads=1):
        def b(e, nnz, k, ops):
            t = [torch.from_numpy(_rnd(60 + i, sh, dt)).to(ops.gpu) for i, sh in enumerate(((M, EN), (k, EN), (k, EN), (M, EN)))]
            d = []
            for sgn in (1.0, -0.5):                               # two consistent data sets: O and lse from the engine's forward
                Q, Kk, V, dO = (x * sgn for x in t)
                O, lse = torch.empty((M, EN), dtype=Q.dtype, device=ops.gpu), torch.empty(_per_head(M, heads), dtype=Q.dtype, device=ops.gpu)
                e.attention(0, Q, Kk, V, O, scale=0.2, bias=True, lse=lse, heads=heads)
                torch.cuda.synchronize()
                d.append((Q, Kk, V, O, dO, lse))
            Q, Kk, V, O, dO, lse = (ops.dense(a, b_) for a, b_ in zip(*d))
            dQ, dK, dV, ds = (ops.out(sh, _tdt(dt)) for sh in ((M, EN), (k, EN), (k, EN), _per_head(nnz, heads)))
            return lambda stream: e.attention_bwd(Q, Kk, V, O, dO, lse, dQ, dK, dV, scale=0.2, bias=True, ds_out=ds, stream=stream,
                                                  heads=heads)
        return b

    def gat(dt, v2, other_heads=False):
        """the engine's GAT (v2: GATv2) forward with `HEADS` heads; other_heads: two GAT calls, 3 heads into outputs of their own and
        then HEADS heads, so that every call of the row sets the narrow exchange up again"""
        def b(e, nnz, k, ops):
            t = _tdt(dt)
            O, lse, p = ops.out((M, EN), t), ops.out((M, HEADS), t), ops.out((nnz, HEADS), t)
            kw = dict(slope=SLOPE, bias=True, lse=lse, p_out=p, heads=HEADS)
            if v2:
                XT, XS, a = (ops.dense(_rnd(63 + i, sh, dt)) for i, sh in enumerate(((M, EN), (k, EN), (HEADS, EN // HEADS))))
                return lambda stream: e.gatv2_attention(0, XT, a, XS, O, stream=stream, **kw)
            el, er, V = (ops.dense(_rnd(66 + i, sh, dt)) for i, sh in enumerate(((M, HEADS), (k, HEADS), (k, EN))))
            if not other_heads:
                return lambda stream: e.gat_attention(0, el, er, V, O, stream=stream, **kw)
            el3, er3 = ops.dense(_rnd(69, (M, 3), dt)), ops.dense(_rnd(70, (k, 3), dt))
            O3, lse3 = ops.out((M, EN), t), ops.out((M, 3), t)

            def call(stream):
                e.gat_attention(0, el3, er3, V, O3, slope=SLOPE, bias=True, lse=lse3, heads=3, stream=stream)
                e.gat_attention(0, el, er, V, O, stream=stream, **kw)
            return call
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
    rows += [("rp-attention-mh-%s" % np.dtype(dt).name, "rp", None, attention(dt, HEADS)) for dt in (F64, F32)]
    rows += [("rp-attention_bwd-mh-%s" % np.dtype(dt).name, "rp", None, attention_bwd(dt, HEADS)) for dt in (F64, F32)]
    rows += [("rp-gat_attention-%s" % np.dtype(dt).name, "rp", None, gat(dt, False)) for dt in (F64, F32)]
    rows += [("rp-gatv2_attention-%s" % np.dtype(dt).name, "rp", None, gat(dt, True)) for dt in (F64, F32)]
    rows += [("rp-exec-timing-on", "rp", "timing-on", exec_(F64)),
             ("rp-gat-other-heads", "rp", "other-heads", gat(F64, False, other_heads=True))]
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
        with _observed(ctx.lib, ctx.reached):
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


def test_every_stream_taking_entry_point_is_reached(ctx, engines):
    """after the rows above (same module, same Ctx): every entry point of both headers that takes a stream and is not in EXEMPT
    was really called by the reference call of some row (_observed), the blocking rows included.  The 2D engine's rows go through
    crp_para2d_*, which have rows of their own; the row engine's entry points are reached by the row engine's rows."""
    if not ctx.reached:                                           # run by itself: the reference call of every row, once
        with _observed(ctx.lib, ctx.reached):
            for name, blocking, build in TABLE:
                ops, call = build(ctx)
                ctx.held.reference(ops, call)
            for name, which, blocking, build in ENGINE_ROWS:
                ops = H.Operands(ctx.gpu)
                e = engines.rp if which == "rp" else engines.p2
                nnz, k = (ctx.ci.size, K) if which == "rp" else (engines.sq[1].size, M)
                ctx.held.reference(ops, build(e, nnz, k, ops))
    for header in ("crpspmm_hip.h", "crp_engine.h"):
        need = stream_entry_points(header) - set(EXEMPT)
        print("%s: %d stream-taking entry points, %d exempt, %d of %d reached by a row"
              % (header, len(need | (set(EXEMPT) & stream_entry_points(header))), len(set(EXEMPT) & stream_entry_points(header)),
                 len(need & ctx.reached), len(need)))
        assert need <= ctx.reached, (header, sorted(need - ctx.reached))


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
