#!/usr/bin/env python3
"""What one call of the fused GAT attention costs against the two ways a caller had before it.  One GPU, one
process, the device handles; every figure is printed as one JSON line.  On the pwtk stand-in and kkt3d(96), in fp64 and fp32, for
H = 4 heads of dv = 8, 16, 64 columns (H dv = 32, 64, 256), the forward:

  gat     one call                                            (crp_gat_attention_csr_*, slope 0.2)
  chain   the unfused chain, per head: sddmm with nk = 2 on Q_h = [el_h, 1], K_h = [1, er_h]; torch's leaky_relu over the nnz
          scores; row_softmax; a value update from the probabilities (fp32: widened to fp64 first, as the update takes them); the
          product with V_h.  It overwrites the handle's values, so it runs on a handle of its own.
  gat1    the same call at slope 1 (the plain additive score)
  dot2    at slope 1 only: the fused dot-product attention with heads = H, dk = 2 on the same Q and K -- the same bits as gat1

The legs alternate in one process; device events around bursts of `--burst` calls after a warm-up of every leg for every shape,
medians over `--reps` bursts, with the bursts' minimum and maximum as the spread of repeated identical runs.  `equal` says that
gat1's O is dot2's bit for bit at the size timed, `chain_diff` is the largest |gat - chain| entry of O.  No ratio is expected in
advance.  Keep the output in profiles/gat_probe.jsonl.

  python tools/gat_probe.py [--matrix pwtk|kkt96|small ...] [--dv 8 16 64] [--heads 4] [--burst 10] [--reps 9]
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
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from crp_spmm_amd import hip
    assert torch.cuda.is_available(), "gat_probe needs a GPU"
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

    for name in a.matrix:
        rp, ci, va = matrix(name)
        rp = np.ascontiguousarray(rp, np.int32)
        ci = np.ascontiguousarray(ci, np.int32)
        m, nnz = rp.size - 1, int(rp[-1])
        A = hip.CsrDev(m, m, rp, ci, va)
        Ac = hip.CsrDev(m, m, rp, ci, va)            # the chain's: its values are overwritten
        for dv in a.dv:
            n = H * dv
            views = [slice(h * dv, (h + 1) * dv) for h in range(H)]
            for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                g = torch.Generator(device=dev)
                g.manual_seed(3)
                el, er = (torch.randn((m, H), dtype=tdt, device=dev, generator=g) for _ in range(2))
                V = torch.randn((m, n), dtype=tdt, device=dev, generator=g)
                Q, K = torch.ones((m, 2 * H), dtype=tdt, device=dev), torch.ones((m, 2 * H), dtype=tdt, device=dev)
                Q[:, 0::2], K[:, 1::2] = el, er
                new = lambda *s: torch.empty(s, dtype=tdt, device=dev)
                Og, Oc, O1, Od = new(m, n), new(m, n), new(m, n), new(m, n)
                s_buf, p_buf = new(nnz), new(nnz)
                spmm = hip.spmm_csr if tdt == torch.float64 else hip.spmm_csr_f32

                def gat():
                    A.gat_attention(el, er, V, slope=0.2, out=Og, heads=H)

                def chain():
                    for h, s in enumerate(views):
                        Ac.sddmm(Q[:, 2 * h:2 * h + 2], K[:, 2 * h:2 * h + 2], out=s_buf)
                        torch.nn.functional.leaky_relu(s_buf, 0.2, inplace=True)
                        Ac.row_softmax(s_buf, out=p_buf)
                        Ac.update_values(p_buf if tdt == torch.float64 else p_buf.double())
                        spmm(Ac, V[:, s], Oc[:, s])

                def gat1():
                    A.gat_attention(el, er, V, slope=1.0, out=O1, heads=H)

                def dot2():
                    A.attention(Q, K, V, scale=1.0, out=Od, heads=H)
                t = timed(dict(gat=gat, chain=chain, gat1=gat1, dot2=dot2))
                torch.cuda.synchronize()
                row = dict(matrix=name, rows=m, nnz=nnz, mean_row=nnz / m, op="forward", heads=H, dv=dv, dtype=tag, burst=a.burst, reps=a.reps,
                           equal=bool(torch.equal(O1, Od)), chain_diff=float((Og - Oc).abs().max()))
                for k, (med, lo, hi) in t.items():
                    row.update({k + "_us": med, k + "_min_us": lo, k + "_max_us": hi})
                row.update(gat_over_chain=t["gat"][0] / t["chain"][0], gat1_over_dot2=t["gat1"][0] / t["dot2"][0])
                print(json.dumps(row), flush=True)
                del el, er, V, Q, K, Og, Oc, O1, Od, s_buf, p_buf
        A.free()
        Ac.free()


if __name__ == "__main__":
    main()
