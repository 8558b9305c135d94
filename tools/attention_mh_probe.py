#!/usr/bin/env python3
"""What one multi-head call of the fused sparse attention costs against the path it replaces: H single-head calls on the column
views of the same tensors.  One GPU, one process, the device handles (CsrDev and its transpose); every figure is
printed as one JSON line.  On the pwtk stand-in and kkt3d(96), in fp64 and fp32, for (H, d) = (8, 32) and (4, 64) -- a layer of
256 columns -- the forward and the backward (row side and column side together):

  mh      one call with heads = H                          (crp_attention_mh_csr_*; crp_attention_bwd_q_mh_csr_* + _bwd_kv_mh_csr_*)
  loop    H calls with nk = nv = d on the views [:, h d:(h + 1) d] of the same tensors, writing the same outputs
  wide    for context only: ONE single-head call at n = H d.  It computes something else (one softmax over 256-wide dots).

The legs alternate in one process; device events around bursts of `--burst` calls after a warm-up of every leg for every shape,
medians over `--reps` bursts, with the bursts' minimum and maximum as the spread of repeated identical runs.  `equal` says that
the mh leg's outputs are the loop leg's bit for bit at the size timed.  No ratio is expected in advance.  Keep the output in
profiles/attention_mh_probe.jsonl.

  python tools/attention_mh_probe.py [--matrix pwtk|kkt96|small ...] [--shape 8x32 4x64] [--burst 10] [--reps 9]
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
    ap.add_argument("--shape", nargs="+", default=["8x32", "4x64"], help="HxD: heads x columns per head")
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from crp_spmm_amd import hip
    assert torch.cuda.is_available(), "attention_mh_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)

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
        for shape in a.shape:
            H, d = (int(x) for x in shape.split("x"))
            n = H * d
            views = [slice(h * d, (h + 1) * d) for h in range(H)]
            for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                g = torch.Generator(device=dev)
                g.manual_seed(3)
                Q, K, V, dO = (torch.randn((m, n), dtype=tdt, device=dev, generator=g) for _ in range(4))
                new = lambda *s: torch.empty(s, dtype=tdt, device=dev)
                scale = 1.0 / np.sqrt(d)
                # ---- forward
                Om, Ol, Ow = new(m, n), new(m, n), new(m, n)
                lse_m, lse_l, lse_w = new(m, H), new(H, m), new(m)

                def fwd_mh():
                    A.attention(Q, K, V, scale=scale, out=Om, lse=lse_m, heads=H)

                def fwd_loop():
                    for h, s in enumerate(views):
                        A.attention(Q[:, s], K[:, s], V[:, s], scale=scale, out=Ol[:, s], lse=lse_l[h])

                def fwd_wide():
                    A.attention(Q, K, V, scale=scale, out=Ow, lse=lse_w)
                tf = timed(dict(mh=fwd_mh, loop=fwd_loop, wide=fwd_wide))
                equal_f = bool(torch.equal(Om, Ol)) and bool(torch.equal(lse_m, lse_l.t()))
                # ---- backward, both sides (O and lse of each leg's own forward)
                outs_m, outs_l, outs_w = ([new(m, n) for _ in range(3)] for _ in range(3))
                dl_m, dl_l, dl_w = new(m, H), new(H, m), new(m)

                def bwd_mh():
                    A.attention_bwd_q(Q, K, V, Om, dO, lse_m, scale=scale, dQ=outs_m[0], delta=dl_m, heads=H)
                    At.attention_bwd_kv(K, V, Q, dO, lse_m, dl_m, scale=scale, dK=outs_m[1], dV=outs_m[2], heads=H)

                def bwd_loop():
                    for h, s in enumerate(views):
                        A.attention_bwd_q(Q[:, s], K[:, s], V[:, s], Ol[:, s], dO[:, s], lse_l[h], scale=scale, dQ=outs_l[0][:, s], delta=dl_l[h])
                    for h, s in enumerate(views):
                        At.attention_bwd_kv(K[:, s], V[:, s], Q[:, s], dO[:, s], lse_l[h], dl_l[h], scale=scale, dK=outs_l[1][:, s],
                                            dV=outs_l[2][:, s])

                def bwd_wide():
                    A.attention_bwd_q(Q, K, V, Ow, dO, lse_w, scale=scale, dQ=outs_w[0], delta=dl_w)
                    At.attention_bwd_kv(K, V, Q, dO, lse_w, dl_w, scale=scale, dK=outs_w[1], dV=outs_w[2])
                tb = timed(dict(mh=bwd_mh, loop=bwd_loop, wide=bwd_wide))
                equal_b = all(bool(torch.equal(x, y)) for x, y in zip(outs_m, outs_l)) and bool(torch.equal(dl_m, dl_l.t()))
                for op, t, equal in (("forward", tf, equal_f), ("backward", tb, equal_b)):
                    print(json.dumps(dict(matrix=name, rows=m, nnz=nnz, mean_row=nnz / m, op=op, heads=H, d=d, dtype=tag, burst=a.burst,
                                          reps=a.reps, mh_us=t["mh"][0], mh_min_us=t["mh"][1], mh_max_us=t["mh"][2], loop_us=t["loop"][0],
                                          loop_min_us=t["loop"][1], loop_max_us=t["loop"][2], mh_over_loop=t["mh"][0] / t["loop"][0],
                                          wide_us=t["wide"][0], wide_min_us=t["wide"][1], wide_max_us=t["wide"][2], equal=equal)),
                          flush=True)
                del Q, K, V, dO, Om, Ol, Ow, lse_m, lse_l, lse_w, outs_m, outs_l, outs_w, dl_m, dl_l, dl_w
        A.free()
        At.free()


if __name__ == "__main__":
    main()
