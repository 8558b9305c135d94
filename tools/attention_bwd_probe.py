#!/usr/bin/env python3
"""What the fused sparse-attention backward costs against the chain of existing calls it replaces.  One GPU, one
process, the row engine on one rank; every figure is printed as one JSON line.  On the pwtk stand-in and kkt3d(96), in fp64 and
fp32, for nk = nv = n in {32, 64, 256}, after one forward that leaves O, lse and the probabilities p:

  fused   RpSpmm.attention_bwd  (crp_attention_bwd_q_csr_* and crp_attention_bwd_kv_csr_*: p re-formed from lse, nothing nnz-sized)
  chain   update_values_dev(p) -> exec_t(dO) = dV;  sddmm(dO, V) = dP;  row_softmax_bwd(p, dP) = dS;  update_values_dev(dS);
          exec(K) = dQ, exec_t(Q) = dK;  two torch multiplies by the scale

-- the chain of tests/test_gpu_attention.py::test_one_backward_step_from_the_existing_calls on the engine.  The two legs alternate
in one process; device events around bursts of `--burst` calls after a warm-up of both legs for every shape, medians over
`--reps` bursts, with the bursts' minimum and maximum as the spread of repeated identical runs.  No ratio is expected in advance.
Keep the output in profiles/attention_bwd_probe.jsonl.

  python tools/attention_bwd_probe.py [--matrix pwtk|kkt96|small ...] [--n 32 64 256] [--burst 10] [--reps 9]
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
    assert torch.cuda.is_available(), "attention_bwd_probe needs a GPU"
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
        va_dev = torch.from_numpy(np.ascontiguousarray(va, np.float64)).to(dev)
        for n in a.n:
            e = engine.RpSpmm(0, m, rp, ci, va, [0, m], n, sc)
            e.set_timing(False)
            for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                g = torch.Generator(device=dev)
                g.manual_seed(3)
                Q, K, V, dO = (torch.randn((m, n), dtype=tdt, device=dev, generator=g) for _ in range(4))
                O = torch.empty((m, n), dtype=tdt, device=dev)
                lse = torch.empty(m, dtype=tdt, device=dev)
                p = torch.empty(nnz, dtype=tdt, device=dev)
                dP, dS = torch.empty_like(p), torch.empty_like(p)
                outs = [torch.empty((m, n), dtype=tdt, device=dev) for _ in range(6)]
                dQf, dKf, dVf, dQc, dKc, dVc = outs
                scale = 1.0 / np.sqrt(n)
                exec_t = e.exec_t if tag == "f64" else e.exec_t_f32
                e.attention(0, Q, K, V, O, scale=scale, lse=lse, p_out=p)

                def fused():
                    e.attention_bwd(Q, K, V, O, dO, lse, dQf, dKf, dVf, scale=scale)

                def chain():
                    e.update_values_dev(p)
                    exec_t(0, dO, dVc)
                    e.sddmm(0, dO, V, dP)
                    e.row_softmax_bwd(p, dP, out=dS)
                    e.update_values_dev(dS)
                    e.exec(0, K, dQc)
                    exec_t(0, Q, dKc)
                    dQc.mul_(scale)
                    dKc.mul_(scale)
                for _ in range(3):
                    fused()
                    chain()
                torch.cuda.synchronize()
                diff = max(float((x - y).abs().max()) for x, y in ((dQf, dQc), (dKf, dKc), (dVf, dVc)))
                tf, tc = [], []
                for _ in range(a.reps):
                    tf.append(burst_ms(fused))
                    tc.append(burst_ms(chain))
                print(json.dumps(dict(matrix=name, rows=m, nnz=nnz, mean_row=nnz / m, n=n, dtype=tag, burst=a.burst, reps=a.reps,
                                      fused_us=median(tf) * 1e3, fused_min_us=min(tf) * 1e3, fused_max_us=max(tf) * 1e3,
                                      chain_us=median(tc) * 1e3, chain_min_us=min(tc) * 1e3, chain_max_us=max(tc) * 1e3,
                                      fused_over_chain=median(tf) / median(tc), max_abs_diff=diff)), flush=True)
                e.update_values_dev(va_dev)                    # the engine's own values again for the next dtype
                del Q, K, V, dO, O, lse, p, dP, dS, outs, dQf, dKf, dVf, dQc, dKc, dVc
            e.free()
    sc.free()


if __name__ == "__main__":
    main()
