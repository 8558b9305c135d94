#!/usr/bin/env python3
"""What the fused GATv2 attention costs, forward and backward, against two legs that existed before it.  One GPU,
one process, the device handles; every figure is printed as one JSON line.  On the pwtk stand-in and kkt3d(96), in fp64 and fp32,
for H = 4 heads of dv = 8, 16, 64 columns (H dv = 32, 64, 256):

  fwd     one forward call                                     (crp_gatv2_attention_csr_*, slope 0.2, with lse)
  bwd     the backward: row side, column side and col_sum      (crp_gatv2_attention_bwd_row / _col_csr_*, crp_col_sum_*)
  chain   the only way a caller had: torch forms leaky_relu(XT[rows] + XS[cols]) a over the edge-gathered nnz x H dv tensors and
          sums every head's dv columns; then per head row_softmax, a value update from the probabilities (fp32: widened to fp64
          first, as the update takes them) and the product with XS_h.  It overwrites the handle's values, so it runs on a handle of
          its own.  A shape whose gathered tensors would not fit the free device memory is skipped, and the row says so.
  attn    the fused dot-product attention with heads = H, dk = dv, Q = XT, K = V = XS: the cost of the same walk with two gathers
          per entry and no LeakyReLU (another function: only the time is compared)
  attn_bwd  its backward (attention_bwd_q and attention_bwd_kv), beside bwd

The legs alternate in one process; device events around bursts of `--burst` calls after a warm-up of every leg for every shape,
medians over `--reps` bursts, with the bursts' minimum and maximum as the spread of repeated identical runs.  `chain_diff` is the
largest |fwd - chain| entry of O.  No ratio is expected in advance.  Keep the output in profiles/gatv2_probe.jsonl.

  python tools/gatv2_probe.py [--matrix pwtk|kkt96|small ...] [--dv 8 16 64] [--heads 4] [--burst 10] [--reps 9]
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
    assert torch.cuda.is_available(), "gatv2_probe needs a GPU"
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
        At = hip.CsrDev.from_transpose(m, m, rp, ci, va)
        Ac = hip.CsrDev(m, m, rp, ci, va)            # the chain's: its values are overwritten
        rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(rp))).to(dev)
        cols = torch.from_numpy(ci.astype(np.int64)).to(dev)
        for dv in a.dv:
            n = H * dv
            views = [slice(h * dv, (h + 1) * dv) for h in range(H)]
            for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                g = torch.Generator(device=dev)
                g.manual_seed(3)
                XT, XS, dO = (torch.randn((m, n), dtype=tdt, device=dev, generator=g) for _ in range(3))
                av = torch.randn((H, dv), dtype=tdt, device=dev, generator=g) / dv ** 0.5
                new = lambda *s: torch.empty(s, dtype=tdt, device=dev)
                Og, Oc, Od = new(m, n), new(m, n), new(m, n)
                lse, lse_d = new(m, H), new(m, H)
                dXT, dap, dXS, delta, da = new(m, n), new(m, n), new(m, n), new(m, H), new(n)
                dQ, dK, dV, delta_d = new(m, n), new(m, n), new(m, n), new(m, H)
                s_buf, p_buf = new(nnz), new(nnz)
                spmm = hip.spmm_csr if tdt == torch.float64 else hip.spmm_csr_f32
                # the chain holds three nnz x H dv tensors at once (two gathers and their sum)
                need = 3 * nnz * n * XT.element_size()
                fits = need < 0.8 * torch.cuda.mem_get_info()[0]

                def fwd():
                    A.gatv2_attention(XT, XS, av, slope=0.2, out=Og, lse=lse, heads=H)

                def bwd():
                    A.gatv2_attention_bwd_row(XT, XS, av, Og, dO, lse, slope=0.2, dXT=dXT, da_part=dap, delta=delta, heads=H)
                    At.gatv2_attention_bwd_col(XS, XT, av, dO, lse, delta, slope=0.2, dXS=dXS, heads=H)
                    hip.col_sum(dap, out=da)

                def chain():
                    z = torch.nn.functional.leaky_relu(XT[rows] + XS[cols], 0.2)
                    sc = (z * av.view(1, n)).view(nnz, H, dv).sum(dim=2)
                    del z
                    for h, s in enumerate(views):
                        s_buf.copy_(sc[:, h])
                        Ac.row_softmax(s_buf, out=p_buf)
                        Ac.update_values(p_buf if tdt == torch.float64 else p_buf.double())
                        spmm(Ac, XS[:, s], Oc[:, s])

                def attn():
                    A.attention(XT, XS, XS, scale=1.0, out=Od, lse=lse_d, heads=H)

                def attn_bwd():
                    A.attention_bwd_q(XT, XS, XS, Od, dO, lse_d, scale=1.0, dQ=dQ, delta=delta_d, heads=H)
                    At.attention_bwd_kv(XS, XS, XT, dO, lse_d, delta_d, scale=1.0, dK=dK, dV=dV, heads=H)
                legs = dict(fwd=fwd, bwd=bwd, attn=attn, attn_bwd=attn_bwd)
                if fits:
                    legs["chain"] = chain
                t = timed(legs)
                torch.cuda.synchronize()
                row = dict(matrix=name, rows=m, nnz=nnz, mean_row=nnz / m, heads=H, dv=dv, dtype=tag, burst=a.burst, reps=a.reps,
                           chain_skipped=(not fits), chain_bytes=need)
                for k, (med, lo, hi) in t.items():
                    row.update({k + "_us": med, k + "_min_us": lo, k + "_max_us": hi})
                row.update(fwd_over_attn=t["fwd"][0] / t["attn"][0], bwd_over_attn_bwd=t["bwd"][0] / t["attn_bwd"][0])
                if fits:
                    row.update(fwd_over_chain=t["fwd"][0] / t["chain"][0], chain_diff=float((Og - Oc).abs().max()))
                print(json.dumps(row), flush=True)
                del XT, XS, dO, av, Og, Oc, Od, lse, lse_d, dXT, dap, dXS, delta, da, dQ, dK, dV, delta_d, s_buf, p_buf
                torch.cuda.empty_cache()
        for h in (A, At, Ac):
            h.free()


if __name__ == "__main__":
    main()
