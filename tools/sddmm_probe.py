#!/usr/bin/env python3
"""What the sampled dense-dense product costs beside the SpMM kernels on the same handle.  One GPU; every
figure is printed as one JSON line and appended to the output file.

For each matrix (the pwtk stand-in, gen.kkt3d_big(96)) and width n (32, 64, 128, 256), alternating in one process and
timed with device events around bursts of --burst calls after a warm-up of every shape:

  sddmm     crp_sddmm_csr_f64, mode 0, aligned operands of ld = n;
  variant1  crp_spmm_csr_f64 forced to variant 1 (CSR row-group): the kernel with the same access pattern -- one lane group
            per row, no sharing between rows, one B row slice per nonzero; its algorithmic bytes are nearly the same
            (8 n nrow written instead of read, 8 nnz not written).  The yardstick;
  variant0  crp_spmm_csr_f64 as auto picks it: what a format-sharing SDDMM kernel could gain at most.

Medians and minima in ms, the ratios sddmm / variant1 and sddmm / variant0 (of the medians), and the achieved rate over the
algorithmic bytes of the SDDMM (4 nnz + 4 (nrow + 1) + 8 n nrow + 8 n (named rows of Y) + 8 nnz).

  python tools/sddmm_probe.py [--matrix pwtk,kkt96|small] [--n 32,64,128,256] [--reps 30] [--burst 10] [--out profiles/sddmm_probe.txt]
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
    ap.add_argument("--matrix", default="pwtk,kkt96")
    ap.add_argument("--n", default="32,64,128,256")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm_probe.txt"))
    a = ap.parse_args()
    import torch
    import crp_spmm_amd
    from crp_spmm_amd import hip
    lib = crp_spmm_amd.load()
    assert torch.cuda.is_available(), "sddmm_probe needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(a.out, "a")

    def out(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.burst):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.burst

    out(what="device", name=torch.cuda.get_device_name(0), library=lib.crp_hip_version().decode(), reps=a.reps, burst=a.burst)
    for mname in a.matrix.split(","):
        rp, ci, va = matrix(mname)
        rp, ci, va = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(va, np.float64)
        m, nnz = rp.size - 1, int(rp[-1])
        named = int(np.unique(ci).size)
        A = hip.CsrDev(m, m, rp, ci, va)
        for n in (int(x) for x in a.n.split(",")):
            rng = np.random.default_rng(n)
            X = torch.from_numpy(rng.standard_normal((m, n))).to(dev)
            Y = torch.from_numpy(rng.standard_normal((m, n))).to(dev)
            Cm = torch.empty((m, n), dtype=torch.float64, device=dev)
            sc = torch.empty(nnz, dtype=torch.float64, device=dev)
            # the C entry points directly, arguments prepared: a burst must not wait for Python between its launches
            st, h, px, py, pc, ps = torch.cuda.current_stream().cuda_stream, A.handle, X.data_ptr(), Y.data_ptr(), Cm.data_ptr(), sc.data_ptr()

            def spmm(variant):
                assert lib.crp_spmm_csr_f64(h, 0, n, py, n, None, 0, pc, n, variant, st) == 0
            runs = {"sddmm": lambda: lib.crp_sddmm_csr_f64(h, n, px, n, py, n, None, 0, ps, None, 0, st),
                    "variant1": lambda: spmm(1), "variant0": lambda: spmm(0)}
            assert runs["sddmm"]() == 0
            for _ in range(5):                                   # warm-up: code objects, the formats of variant 0
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            ts = {k: [] for k in runs}
            for _ in range(a.reps):
                for k, fn in runs.items():
                    ts[k].append(one(fn))
            v0 = int(lib.crp_csr_dev_last_variant(A.handle))
            med = {k: median(v) for k, v in ts.items()}
            alg = 4 * nnz + 4 * (m + 1) + 8 * n * m + 8 * n * named + 8 * nnz
            out(what="sddmm", matrix=mname, rows=m, nnz=nnz, n=n, sddmm_ms=med["sddmm"], variant1_ms=med["variant1"],
                variant0_ms=med["variant0"], sddmm_min_ms=min(ts["sddmm"]), variant1_min_ms=min(ts["variant1"]),
                variant0_min_ms=min(ts["variant0"]), variant0_resolved=v0, sddmm_over_variant1=med["sddmm"] / med["variant1"],
                sddmm_over_variant0=med["sddmm"] / med["variant0"], sddmm_alg_bytes=alg, sddmm_alg_GBps=alg / med["sddmm"] * 1e-6,
                sddmm_spread=(max(ts["sddmm"]) - min(ts["sddmm"])) / med["sddmm"],
                variant1_spread=(max(ts["variant1"]) - min(ts["variant1"])) / med["variant1"])
            del X, Y, Cm, sc
        A.free()
    log.close()


if __name__ == "__main__":
    main()
