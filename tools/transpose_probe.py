#!/usr/bin/env python3
"""What C := A^T * B costs beside C := A * B.  One GPU; every figure is printed as one JSON line.

  transpose   crp_csr_transpose on the device (arrays already in HBM, wall clock around the call, which synchronises)
              against the host path, and against crp_csr_dev_create_t / crp_csr_dev_create as a whole;
  update      crp_csr_dev_update_values on a transposed handle (the gather through tmap) against a plain handle, from a host
              and from a device pointer, with the team format of n = 256 built;
  accumulate  crp_scatter_add_rows_f64 over the rows rank 0 of a 2-rank row partition sends in the forward exchange (the
              halo that comes back in the transposed product), n = 256, device events;
  product     the product on the transposed handle against the forward product, n = 256, device events, alternating.

  python tools/transpose_probe.py [--matrix pwtk|kkt96|small] [--n 256] [--reps 20]
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
    ap.add_argument("--matrix", default="pwtk")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import crp_spmm_amd
    from crp_spmm_amd import hip, planner
    lib = crp_spmm_amd.load()
    assert torch.cuda.is_available(), "transpose_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rp, ci, va = matrix(a.matrix)
    rp, ci, va = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(va, np.float64)
    m = rp.size - 1
    nnz = int(rp[-1])
    n = a.n
    va = va * (1.0 + 0.37 * np.sin(np.arange(nnz)))      # A != A^T in value; the pattern stays symmetric
    head = dict(matrix=a.matrix, rows=m, nnz=nnz, n=n)

    def out(what, **kw):
        print(json.dumps(dict(head, what=what, **kw)), flush=True)

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def events(fn, reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return ts

    # ---- transpose: device against host
    d_rp, d_ci, d_va = (torch.from_numpy(x).to(dev) for x in (rp, ci, va))
    hip.csr_transpose(d_rp, d_ci, d_va, m)                                   # warm-up: code objects
    t_dev = wall(lambda: hip.csr_transpose(d_rp, d_ci, d_va, m), 5)
    t_host = wall(lambda: hip.csr_transpose(rp, ci, va, m), 3)
    got = [t.cpu().numpy() for t in hip.csr_transpose(d_rp, d_ci, d_va, m)]
    want = hip.csr_transpose(rp, ci, va, m)
    same = all(np.array_equal(g, w) for g, w in zip(got, want))
    out("transpose", device_ms=median(t_dev), device_ms_all=t_dev, host_ms=median(t_host), host_ms_all=t_host, bit_identical=same)
    rp_t, ci_t, va_t, _ = want
    t0 = time.perf_counter()
    At = hip.CsrDev.from_transpose(m, m, rp, ci, va)
    t_ct = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    A = hip.CsrDev(m, m, rp, ci, va)
    t_c = (time.perf_counter() - t0) * 1e3
    out("create", create_t_ms=t_ct, create_ms=t_c)
    del d_rp, d_ci, d_va

    # ---- product: transposed against forward, alternating
    B = torch.from_numpy(np.random.default_rng(1).standard_normal((m, n))).to(dev)
    Cf, Ct = torch.empty((m, n), dtype=torch.float64, device=dev), torch.empty((m, n), dtype=torch.float64, device=dev)
    for _ in range(3):
        hip.spmm_csr(A, B, Cf)
        hip.spmm_csr(At, B, Ct)
    tf, tt = [], []
    for _ in range(a.reps):
        tf += events(lambda: hip.spmm_csr(A, B, Cf), 1)
        tt += events(lambda: hip.spmm_csr(At, B, Ct), 1)
    out("product", forward_ms=median(tf), transposed_ms=median(tt), forward_min_ms=min(tf), transposed_min_ms=min(tt),
        forward_variant=int(lib.crp_csr_dev_last_variant(A.handle)), transposed_variant=int(lib.crp_csr_dev_last_variant(At.handle)),
        forward_reordered=int(lib.crp_csr_dev_reordered(A.handle)), transposed_reordered=int(lib.crp_csr_dev_reordered(At.handle)))

    # ---- update_values, the team format of this width built by the products above
    new = 2.0 * va + 1.0
    d_new = torch.from_numpy(new).to(dev)
    res = {}
    for tag, h in (("plain", A), ("transposed", At)):
        h.update_values(new)
        h.update_values(d_new)
        res[tag + "_host_ms"] = median(wall(lambda: h.update_values(new), 5))
        res[tag + "_device_ms"] = median(wall(lambda: h.update_values(d_new), 5))
    out("update_values", **res)

    # ---- accumulate over the world-2 halo of rank 0
    rb = planner.csr_mat_row_partition(rp, 2)
    cut = int(rb[1])
    cols = np.unique(ci[rp[cut]:])                        # columns the second rank's rows name ...
    halo = cols[cols < cut].astype(np.int32)              # ... inside the first rank's block: it sends them, they come back
    if halo.size:
        seg_row = torch.from_numpy(halo).to(dev)
        seg_ptr = torch.arange(halo.size + 1, dtype=torch.int32, device=dev)
        seg_pos = torch.arange(halo.size, dtype=torch.int32, device=dev)
        src = torch.ones((halo.size, n), dtype=torch.float64, device=dev)
        dst = torch.zeros((cut, n), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def acc():
            rc = lib.crp_scatter_add_rows_f64(int(halo.size), n, seg_row.data_ptr(), seg_ptr.data_ptr(), seg_pos.data_ptr(),
                                              src.data_ptr(), n, dst.data_ptr(), n, C.c_void_p(st))
            assert rc == 0
        for _ in range(3):
            acc()
        ta = events(acc, a.reps)
        out("accumulate", halo_rows=int(halo.size), accumulate_us=median(ta) * 1e3, accumulate_min_us=min(ta) * 1e3,
            bytes_moved=int(halo.size) * n * 8 * 3)
    else:
        out("accumulate", halo_rows=0)
    A.free()
    At.free()


if __name__ == "__main__":
    main()
