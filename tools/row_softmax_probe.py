#!/usr/bin/env python3
"""What the row softmax over A's pattern and its backward cost.  One GPU, one process; every figure is printed
as one JSON line.  On the pwtk stand-in and kkt3d(96), in fp64 and fp32:

  forward   crp_row_softmax_* over the matrix's rows (reads s and the row pointer, writes y: 2 nnz sizeof(T) + 4 (nrow + 1)
            bytes) against a device-to-device copy that reads plus writes the same number of bytes (crp_dev_memcpy of half of
            them: code that exists before this kernel);
  backward  crp_row_softmax_bwd_* (reads y and dy, writes ds: 3 nnz sizeof(T) + 4 (nrow + 1) bytes) against such a copy.

The legs of a pair alternate in one process; device events around bursts of `--burst` calls after a warm-up of both legs,
medians over `--reps` bursts.  No ratio is expected in advance: nobody has measured this kernel.  Keep the output in
profiles/row_softmax_probe.jsonl.

  python tools/row_softmax_probe.py [--matrix pwtk|kkt96|small ...] [--burst 20] [--reps 9]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    import crp_spmm_amd
    from crp_spmm_amd import hip
    lib = crp_spmm_amd.load()
    assert torch.cuda.is_available(), "row_softmax_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def burst_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.burst):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.burst

    def pair(f, g):
        for _ in range(3):
            f()
            g()
        torch.cuda.synchronize()
        tf, tg = [], []
        for _ in range(a.reps):
            tf.append(burst_ms(f))
            tg.append(burst_ms(g))
        return tf, tg

    for name in a.matrix:
        rp = np.ascontiguousarray(matrix(name)[0], np.int32)
        m, nnz = rp.size - 1, int(rp[-1])
        rp_d = torch.from_numpy(rp).to(dev)
        lens = np.diff(rp)
        for tdt, isz, tag in ((torch.float64, 8, "f64"), (torch.float32, 4, "f32")):
            rng = np.random.default_rng(3)
            s = torch.from_numpy(rng.uniform(-8, 0, nnz)).to(dev).to(tdt)
            dy = torch.from_numpy(rng.standard_normal(nnz)).to(dev).to(tdt)
            y, ds = torch.empty_like(s), torch.empty_like(s)
            hip.row_softmax(rp_d, s, out=y)
            for what, nvec, fn in (("forward", 2, lambda: hip.row_softmax(rp_d, s, out=y)),
                                   ("backward", 3, lambda: hip.row_softmax_bwd(rp_d, y, dy, out=ds))):
                nbytes = nvec * nnz * isz + 4 * (m + 1)
                half = nbytes // 2 // 16 * 16
                c_src = torch.empty(half, dtype=torch.uint8, device=dev)
                c_dst = torch.empty(half, dtype=torch.uint8, device=dev)

                def copy_():
                    rc = lib.crp_dev_memcpy(c_dst.data_ptr(), c_src.data_ptr(), half, 2, st)
                    assert rc == 0, rc
                tk, tc = pair(fn, copy_)
                print(json.dumps(dict(matrix=name, rows=m, nnz=nnz, mean_row=nnz / m, max_row=int(lens.max()), dtype=tag, what=what,
                                      burst=a.burst, reps=a.reps, bytes_read_plus_written=nbytes, kernel_us=median(tk) * 1e3,
                                      kernel_min_us=min(tk) * 1e3, kernel_max_us=max(tk) * 1e3, kernel_GBps=nbytes / median(tk) / 1e6,
                                      copy_us=median(tc) * 1e3, copy_min_us=min(tc) * 1e3, copy_max_us=max(tc) * 1e3,
                                      copy_GBps=2 * half / median(tc) / 1e6, kernel_over_copy=median(tk) / median(tc))), flush=True)
                del c_src, c_dst
            del s, dy, y, ds


if __name__ == "__main__":
    main()
