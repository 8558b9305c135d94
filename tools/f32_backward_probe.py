#!/usr/bin/env python3
"""What the fp32 transposed product and the device-resident value update cost.  One GPU, one process; every
figure is printed as one JSON line.  Three pairs, each against code that existed before them:

  exec_t      RpSpmm.exec_t_f32 against RpSpmm.exec on float32 operands, on the same one-rank engine, n columns.  The pwtk
              stand-in is structurally symmetric, so A and A^T get the same formats and the same kernel there;
  accumulate  crp_scatter_add_rows_f32 over the rows rank 0 of a 2-rank row partition sends in the forward exchange (the halo
              that comes back in the transposed product) against a device-to-device copy of the same number of bytes, read
              plus written (3 * rows * n * 4, so the copy moves half of that each way);
  update      RpSpmm.update_values_dev (fp64 values in HBM) against RpSpmm.update_values (the same values on the host), in
              wall time around a call plus a device synchronisation: the host path blocks, the device path is asynchronous.

The legs of a pair alternate in one process; device events around bursts of `--burst` calls after a warm-up of both legs,
medians over `--reps` bursts (the update pair: wall clock, one call per measurement).  No ratio is expected in advance.

  python tools/f32_backward_probe.py [--matrix pwtk|kkt96|small ...] [--n 256] [--burst 10] [--reps 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import crp_spmm_amd
    from crp_spmm_amd import comm, engine, planner
    lib = crp_spmm_amd.load()
    assert torch.cuda.is_available(), "f32_backward_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    n = a.n
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

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name in a.matrix:
        rp, ci, va = matrix(name)
        rp, ci, va = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(va, np.float64)
        m, nnz = rp.size - 1, int(rp[-1])
        head = dict(matrix=name, rows=m, nnz=nnz, n=n, burst=a.burst, reps=a.reps)

        def out(what, **kw):
            print(json.dumps(dict(head, what=what, **kw)), flush=True)

        # ---- exec_t_f32 against the fp32 exec on one engine
        sc = comm.SelfComm()
        e = engine.RpSpmm(0, m, rp, ci, va, [0, m], n, sc)
        e.set_timing(False)
        B = torch.from_numpy(np.random.default_rng(1).standard_normal((m, n)).astype(np.float32)).to(dev)
        Cf, Ct = torch.empty((m, n), dtype=torch.float32, device=dev), torch.empty((m, n), dtype=torch.float32, device=dev)
        tf, tt = pair(lambda: e.exec(0, B, Cf), lambda: e.exec_t_f32(0, B, Ct))
        fwd_kernel = e.kernel_info()["variant_name"]
        out("exec_t", exec_f32_us=median(tf) * 1e3, exec_f32_min_us=min(tf) * 1e3, exec_f32_max_us=max(tf) * 1e3,
            exec_t_f32_us=median(tt) * 1e3, exec_t_f32_min_us=min(tt) * 1e3, exec_t_f32_max_us=max(tt) * 1e3,
            exec_t_over_exec=median(tt) / median(tf), forward_kernel=fwd_kernel)

        # ---- update_values_dev against update_values, wall time; the forward and the transposed formats exist
        new = 2.0 * va + 1.0
        d_new = torch.from_numpy(new).to(dev)
        for _ in range(2):
            e.update_values(new)
            e.update_values_dev(d_new)
        th, td, tdi = [], [], []
        for _ in range(a.reps):
            th.append(wall_ms(lambda: e.update_values(new)))
            td.append(wall_ms(lambda: e.update_values_dev(d_new)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.update_values_dev(d_new)
            tdi.append((time.perf_counter() - t0) * 1e3)              # the call alone: what the host waits
        torch.cuda.synchronize()
        out("update", host_ms=median(th), host_min_ms=min(th), host_max_ms=max(th), device_ms=median(td), device_min_ms=min(td),
            device_max_ms=max(td), device_call_ms=median(tdi), host_over_device=median(th) / median(td), value_bytes=8 * nnz)
        e.free()
        sc.free()
        del B, Cf, Ct, d_new

        # ---- the accumulate over the world-2 halo of rank 0 against a copy of the same bytes
        rb = planner.csr_mat_row_partition(rp, 2)
        cut = int(rb[1])
        cols = np.unique(ci[rp[cut]:])
        halo = cols[cols < cut].astype(np.int32)
        if halo.size:
            h = int(halo.size)
            seg_row = torch.from_numpy(halo).to(dev)
            seg_ptr = torch.arange(h + 1, dtype=torch.int32, device=dev)
            seg_pos = torch.arange(h, dtype=torch.int32, device=dev)
            src = torch.ones((h, n), dtype=torch.float32, device=dev)
            dst = torch.zeros((cut, n), dtype=torch.float32, device=dev)
            nbytes = 3 * h * n * 4
            half = nbytes // 2 // 16 * 16
            c_src = torch.empty(half, dtype=torch.uint8, device=dev)
            c_dst = torch.empty(half, dtype=torch.uint8, device=dev)

            def acc():
                rc = lib.crp_scatter_add_rows_f32(h, n, seg_row.data_ptr(), seg_ptr.data_ptr(), seg_pos.data_ptr(), src.data_ptr(), n,
                                                  dst.data_ptr(), n, st)
                assert rc == 0, rc

            def copy_():
                rc = lib.crp_dev_memcpy(c_dst.data_ptr(), c_src.data_ptr(), half, 2, st)
                assert rc == 0, rc
            ta, tc = pair(acc, copy_)
            out("accumulate", halo_rows=h, bytes_read_plus_written=nbytes, accumulate_us=median(ta) * 1e3, accumulate_min_us=min(ta) * 1e3,
                accumulate_max_us=max(ta) * 1e3, accumulate_GBps=nbytes / median(ta) / 1e6, copy_us=median(tc) * 1e3,
                copy_min_us=min(tc) * 1e3, copy_max_us=max(tc) * 1e3, copy_GBps=2 * half / median(tc) / 1e6,
                accumulate_over_copy=median(ta) / median(tc))
            del seg_row, seg_ptr, seg_pos, src, dst, c_src, c_dst
        else:
            out("accumulate", halo_rows=0)


if __name__ == "__main__":
    main()
