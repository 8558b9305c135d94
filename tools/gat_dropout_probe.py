#!/usr/bin/env python3
"""What attention dropout costs in the fused GAT and GATv2 calls, and what a caller had before it.  One GPU, one
process, the device handles; every figure is printed as one JSON line.  On the pwtk stand-in and kkt3d(96), in fp64 and fp32, for
H = 4 heads of dv = 8, 16, 64 columns, for both layers, forward and backward (row side + column side, GATv2 with col_sum):

  drop    the call at rate 0.6                                  (crp_gat_attention_drop_*, crp_gatv2_attention_drop_*)
  plain   the same call at rate 0: the kernel of the parent commit, so drop / plain is what the draw and the two products cost
  chain   forward only, what a caller had at the parent commit: the fused forward with p_out, torch's dropout over the (nnz, H)
          probabilities, and per head a value update (fp32: widened to fp64 first, as the update takes them) on a handle of its
          own and the product with that head's columns of V / XS

The legs alternate in one process; device events around bursts of `--burst` calls after a warm-up of every leg for every shape,
medians over `--reps` bursts, with the bursts' minimum and maximum as the spread of repeated identical runs.  No ratio is expected
in advance.  Keep the output in profiles/gat_dropout_probe.jsonl.

  python tools/gat_dropout_probe.py [--matrix pwtk|kkt96|small ...] [--dv 8 16 64] [--heads 4] [--rate 0.6] [--burst 10] [--reps 9]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def matrix(name):
    from crp_spmm_amd import gen
    if name == "pwtk":
        return gen.banded_fem(217918)
    if name == "kkt96":
        return gen.kkt3d_big(96)
    if name == "small":
        return gen.banded_fem(6000, offsets=(1, 2, 3, 4, 50, 51, 1400))
    raise SystemExit("unknown matrix %r" % name)


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", nargs="+", default=["pwtk", "kkt96"])
    ap.add_argument("--dv", nargs="+", type=int, default=[8, 16, 64], help="columns per head")
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--rate", type=float, default=0.6)
    ap.add_argument("--seed", type=int, default=0x1234567800000001)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from crp_spmm_amd import hip
    assert torch.cuda.is_available(), "gat_dropout_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    H = a.heads

    def burst_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.burst):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.burst

    def timed(legs):
        """legs: name -> callable.  Warm up all, then alternate them; name -> (median, min, max) in microseconds"""
        for _ in range(3):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, fn in legs.items():
                t[k].append(burst_ms(fn))
        return {k: (median(v) * 1e3, min(v) * 1e3, max(v) * 1e3) for k, v in t.items()}

    def emit(base, t, **extra):
        row = dict(base, **extra)
        for k, (med, lo, hi) in t.items():
            row.update({k + "_us": med, k + "_min_us": lo, k + "_max_us": hi})
        row["drop_over_plain"] = t["drop"][0] / t["plain"][0]
        if "chain" in t:
            row["drop_over_chain"] = t["drop"][0] / t["chain"][0]
        print(json.dumps(row), flush=True)

    for name in a.matrix:
        rp, ci, va = matrix(name)
        rp = np.ascontiguousarray(rp, np.int32)
        ci = np.ascontiguousarray(ci, np.int32)
        m, nnz = rp.size - 1, int(rp[-1])
        A = hip.CsrDev(m, m, rp, ci, va)
        At = hip.CsrDev.from_transpose(m, m, rp, ci, va)
        Ac = hip.CsrDev(m, m, rp, ci, va)            # the chain's: its values are overwritten
        for dv in a.dv:
            n = H * dv
            views = [slice(h * dv, (h + 1) * dv) for h in range(H)]
            for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                g = torch.Generator(device=dev)
                g.manual_seed(3)
                el, er = (torch.randn((m, H), dtype=tdt, device=dev, generator=g) for _ in range(2))
                V, XT, dO = (torch.randn((m, n), dtype=tdt, device=dev, generator=g) for _ in range(3))
                av = torch.randn((H, dv), dtype=tdt, device=dev, generator=g) / dv ** 0.5
                new = lambda *s: torch.empty(s, dtype=tdt, device=dev)
                O, Oc, lse, p_buf = new(m, n), new(m, n), new(m, H), new(nnz, H)
                d_el, d_er, delta, dV, dXT, dap = new(m, H), new(m, H), new(m, H), new(m, n), new(m, n), new(m, n)
                spmm = hip.spmm_csr if tdt == torch.float64 else hip.spmm_csr_f32
                base = dict(matrix=name, rows=m, nnz=nnz, mean_row=nnz / m, heads=H, dv=dv, dtype=tag, rate=a.rate, burst=a.burst, reps=a.reps)

                def chain_tail():
                    pd = torch.nn.functional.dropout(p_buf, a.rate)
                    for h, s in enumerate(views):
                        col = pd[:, h].contiguous()
                        Ac.update_values(col if tdt == torch.float64 else col.double())
                        spmm(Ac, V[:, s], Oc[:, s])

                for layer in ("gat", "gatv2"):
                    if layer == "gat":
                        fwd = lambda r, **kw: A.gat_attention(el, er, V, slope=0.2, out=O, lse=lse, heads=H, dropout=r, seed=a.seed, **kw)

                        def bwd(r):
                            A.gat_attention_bwd_row(el, er, V, O, dO, lse, slope=0.2, d_el=d_el, delta=delta, heads=H, dropout=r, seed=a.seed)
                            At.gat_attention_bwd_col(er, V, el, dO, lse, delta, slope=0.2, d_er=d_er, dV=dV, heads=H, dropout=r, seed=a.seed)
                    else:
                        fwd = lambda r, **kw: A.gatv2_attention(XT, V, av, slope=0.2, out=O, lse=lse, heads=H, dropout=r, seed=a.seed, **kw)

                        def bwd(r):
                            A.gatv2_attention_bwd_row(XT, V, av, O, dO, lse, slope=0.2, dXT=dXT, da_part=dap, delta=delta, heads=H, dropout=r,
                                                      seed=a.seed)
                            At.gatv2_attention_bwd_col(V, XT, av, dO, lse, delta, slope=0.2, dXS=dV, heads=H, dropout=r, seed=a.seed)
                            hip.col_sum(dap)

                    def chain():
                        fwd(0.0, p_out=p_buf)
                        chain_tail()
                    t = timed(dict(drop=lambda: fwd(a.rate), plain=lambda: fwd(0.0), chain=chain))
                    emit(base, t, layer=layer, op="forward")
                    fwd(a.rate)                       # O and lse of the dropped forward: what the backward legs read
                    t = timed(dict(drop=lambda: bwd(a.rate), plain=lambda: bwd(0.0)))
                    emit(base, t, layer=layer, op="backward")
                torch.cuda.synchronize()
                del el, er, V, XT, dO, av, O, Oc, lse, p_buf, d_el, d_er, delta, dV, dXT, dap
        A.free()
        At.free()
        Ac.free()


if __name__ == "__main__":
    main()
