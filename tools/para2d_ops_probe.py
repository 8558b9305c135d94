#!/usr/bin/env python3
"""What the grid-row sum of the 2D engine's SDDMM costs.  One GPU; every figure is printed as one JSON line.

  crp_sum_segments_f64 / _f32 for nseg = 2, 4, 8 at the nonzero count of the pwtk stand-in (the slice a rank of a 1 x pn
  grid would sum is smaller: this is the upper end), against a device-to-device copy of the SAME number of bytes, read plus
  written -- (nseg + 1) * len * itemsize, so the copy moves half of that.  Both alternate in one process; device events
  around bursts of `--burst` calls after a warm-up of both.  No ratio is expected in advance: the kernel reads nseg
  streams and writes one, the copy reads one and writes one.

  python tools/para2d_ops_probe.py [--len 11102984] [--burst 20] [--reps 7]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

PWTK_STANDIN_NNZ = 11102984         # gen.banded_fem(217918)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len", type=int, default=PWTK_STANDIN_NNZ)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import crp_spmm_amd
    lib = crp_spmm_amd.load()
    assert torch.cuda.is_available(), "para2d_ops_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ln = a.len
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def burst_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.burst):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.burst

    for name, tdt, isz, fn in (("f64", torch.float64, 8, lib.crp_sum_segments_f64), ("f32", torch.float32, 4, lib.crp_sum_segments_f32)):
        for nseg in (2, 4, 8):
            src = torch.rand(nseg * ln, dtype=tdt, device=dev)
            out = torch.empty(ln, dtype=tdt, device=dev)
            nbytes = (nseg + 1) * ln * isz                          # what the sum reads plus writes
            half = nbytes // 2 // 16 * 16                           # the copy reads and writes this much each
            c_src = torch.empty(half, dtype=torch.uint8, device=dev)
            c_dst = torch.empty(half, dtype=torch.uint8, device=dev)

            def sum_():
                rc = fn(nseg, ln, src.data_ptr(), ln, out.data_ptr(), st)
                assert rc == 0, rc

            def copy_():
                rc = lib.crp_dev_memcpy(c_dst.data_ptr(), c_src.data_ptr(), half, 2, st)
                assert rc == 0, rc
            for _ in range(3):
                sum_()
                copy_()
            torch.cuda.synchronize()
            want = src.view(nseg, ln)[0].clone()
            for j in range(1, nseg):
                want = want + src.view(nseg, ln)[j]
            same = bool(torch.equal(out, want))
            ts, tc = [], []
            for _ in range(a.reps):
                ts.append(burst_ms(sum_))
                tc.append(burst_ms(copy_))
            ms, mc = float(np.median(ts)), float(np.median(tc))
            print(json.dumps(dict(what="sum_segments", dtype=name, nseg=nseg, len=ln, bytes_read_plus_written=nbytes,
                                  sum_us=ms * 1e3, sum_min_us=min(ts) * 1e3, sum_max_us=max(ts) * 1e3, sum_GBps=nbytes / ms / 1e6,
                                  copy_us=mc * 1e3, copy_min_us=min(tc) * 1e3, copy_max_us=max(tc) * 1e3, copy_GBps=2 * half / mc / 1e6,
                                  sum_over_copy=ms / mc, left_to_right=same, burst=a.burst, reps=a.reps)), flush=True)
            del src, out, c_src, c_dst


if __name__ == "__main__":
    main()
