#!/usr/bin/env python3
"""What the fused sparse attention costs against the chain it replaces.  One GPU, one process, the row engine on
one rank; every figure is printed as one JSON line.  On the pwtk stand-in and kkt3d(96), in fp64 and fp32, for
nk = nv = n in {32, 64, 256}:

  fused   RpSpmm.attention  (crp_attention_csr_*: scores, online softmax and the product with V in one trip over the row)
  chain   RpSpmm.sddmm -> scale (one torch multiply over the nnz scores) -> row_softmax -> update_values_dev -> exec

The two legs alternate in one process; device events around bursts of `--burst` calls after a warm-up of both legs for every
shape, medians over `--reps` bursts, with the bursts' minimum and maximum as the spread of repeated identical runs.  Reported per
leg: time, the algorithmic bytes 4 nnz + 4 (m + 1) + T (m nk + m nv + distinct rows (nk + nv)) -- the column indices, the row
pointer, Q in and O out, every named row of K and V once -- and the rate on them.  No ratio is expected in advance.  Keep the
output in profiles/attention_probe.jsonl.

  python tools/attention_probe.py [--matrix pwtk|kkt96|small ...] [--n 32 64 256] [--burst 10] [--reps 9]
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
    ap.add_argument("--n", nargs="+", type=int, default=[32, 64, 256])
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from crp_spmm_amd import comm, engine
    assert torch.cuda.is_available(), "attention_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    sc = comm.SelfComm()

    def burst_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.burst):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.burst

    for name in a.matrix:
        rp, ci, va = matrix(name)
        rp = np.ascontiguousarray(rp, np.int32)
        m, nnz = rp.size - 1, int(rp[-1])
        distinct = int(np.unique(ci).size)
        for n in a.n:
            e = engine.RpSpmm(0, m, rp, ci, va, [0, m], n, sc)
            e.set_timing(False)
            for tdt, isz, tag in ((torch.float64, 8, "f64"), (torch.float32, 4, "f32")):
                g = torch.Generator(device=dev)
                g.manual_seed(3)
                Q, K, V = (torch.randn((m, n), dtype=tdt, device=dev, generator=g) for _ in range(3))
                O = torch.empty((m, n), dtype=tdt, device=dev)
                C = torch.empty((m, n), dtype=tdt, device=dev)
                s = torch.empty(nnz, dtype=tdt, device=dev)
                scale = 1.0 / np.sqrt(n)

                def fused():
                    e.attention(0, Q, K, V, O, scale=scale)

                def chain():
                    e.sddmm(0, Q, K, s)
                    s.mul_(scale)
                    e.row_softmax(s, out=s)
                    e.update_values_dev(s)
                    e.exec(0, V, C)
                for _ in range(3):
                    fused()
                    chain()
                torch.cuda.synchronize()
                diff = float((O - C).abs().max())
                tf, tc = [], []
                for _ in range(a.reps):
                    tf.append(burst_ms(fused))
                    tc.append(burst_ms(chain))
                nbytes = 4 * nnz + 4 * (m + 1) + isz * (2 * m * n + distinct * 2 * n)
                print(json.dumps(dict(matrix=name, rows=m, nnz=nnz, mean_row=nnz / m, n=n, dtype=tag, burst=a.burst, reps=a.reps,
                                      algorithmic_bytes=nbytes, fused_us=median(tf) * 1e3, fused_min_us=min(tf) * 1e3,
                                      fused_max_us=max(tf) * 1e3, fused_GBps=nbytes / median(tf) / 1e6, chain_us=median(tc) * 1e3,
                                      chain_min_us=min(tc) * 1e3, chain_max_us=max(tc) * 1e3, chain_GBps=nbytes / median(tc) / 1e6,
                                      fused_over_chain=median(tf) / median(tc), max_abs_diff=diff)), flush=True)
                del Q, K, V, O, C, s
            e.free()
    sc.free()


if __name__ == "__main__":
    main()
