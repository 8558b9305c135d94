"""GPU: the row-parallel engine's fused GATv2 attention on 2 and 4 ranks that share one GPU (tests/gpu_dist_gatv2_worker.py states what
is held): O, lse and p_out bit-identical to the handle call on the whole matrix across rank counts, timing modes, layouts, host
and device operands and repeated calls; and, at one rank in this process, the stream contract of DESIGN.md 5m on a held-back
non-blocking side stream (tests/streams_harness.py): order, asynchrony and the control."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 4])
def test_multi_rank_one_gpu(world):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    env.pop("CRPSPMM_EXPECT_NATIVE_RCCL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(30390 + world), os.path.join(ROOT, "tests", "gpu_dist_gatv2_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_GATV2_WORKER_OK world=%d" % world in r.stdout


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_rank_equals_the_handle_and_obeys_the_stream_contract(crp, gpu, dtype):
    """world 1, timing off, device operands: ``gatv2_built`` reads False, then True; the engine's O, lse and p_out are the handle
    call's; on the held-back side stream the call gives the default stream's bits (order) and returns while the stream is still held
    (asynchrony); told to use the null stream under the same hold-back it does not (control)"""
    import torch
    import streams_harness as SH
    from crp_spmm_amd import comm, engine, gen, hip
    m, k, n, H = 300, 260, 24, 3
    rp, ci, va = gen.random_csr(m, k, 9, seed=4, empty_every=11)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    nnz = ci.size
    rng = np.random.default_rng(8)
    tdt = torch.float64 if dtype == "float64" else torch.float32
    XT, av, V = (rng.standard_normal(s).astype(dtype) for s in ((m, n), (H, n // H), (k, n)))
    av = (av / np.sqrt(n // H)).astype(dtype)
    A = hip.CsrDev(m, k, rp, ci, va)
    xtd, avd, Vd = (torch.from_numpy(x).to(gpu) for x in (XT, av, V))
    lse0, p0 = torch.empty((m, H), dtype=tdt, device=gpu), torch.empty((nnz, H), dtype=tdt, device=gpu)
    O0 = A.gatv2_attention(xtd, Vd, avd, slope=0.2, bias=True, lse=lse0, p_out=p0, heads=H)
    torch.cuda.synchronize()
    sc = comm.SelfComm()
    e = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
    e.set_timing(False)
    held = SH.Held(crp.load())
    try:
        assert e.gatv2_built() is False
        ops = SH.Operands(gpu)
        a, b, v = ops.dense(XT), ops.dense(av), ops.dense(V)
        O, lse, p = ops.out((m, n), tdt), ops.out((m, H), tdt), ops.out((nnz, H), tdt)
        call = lambda stream: e.gatv2_attention(0, a, b, v, O, slope=0.2, bias=True, lse=lse, p_out=p, heads=H, stream=stream)
        want = held.reference(ops, call)
        assert e.gatv2_built() is True
        assert SH.same(want, [O0, lse0, p0]), "the engine at one rank against the handle call"
        held.warm(ops, call)
        got, pending = held.run(ops, call)
        assert SH.same(got, want), "Order"
        assert pending, "Asynchrony"
        bad, _ = held.run(ops, call, stream=0)
        held.heal(ops, call)
        assert not SH.same(bad, want), "Control"
    finally:
        held.close()
        e.free()
        sc.free()
        A.free()
