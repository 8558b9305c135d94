"""GPU: the fp32 exec of the row-parallel and 2D engines (crp_rp_spmm_exec_f32_ex / crp_para2d_spmm_exec_f32_ex), its
packing and transpose kernels (crp_gather_rows_f32 / crp_scatter_rows_f32 / crp_transpose_f32), and -- through
tests/gpu_dist_f32_worker.py -- the fp32 exchange with 2 and 4 ranks sharing the card."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import FP64_TOL, ROOT

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-5          # fp32 parity bar against the fp64 oracle (tests/test_gpu_parity.py)
WIDTHS = (1, 3, 24, 30, 64, 128, 256)


def _cases():
    from crp_spmm_amd import gen
    rp, ci, va = gen.fem3d(12)
    m = len(rp) - 1
    yield "fem3d", rp, ci, va, max(int(ci.max()) + 1, m)
    rp, ci, va = gen.random_csr(777, 1234, 70, seed=11, empty_every=13)
    yield "random", rp, ci, va, 1234


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _padded(torch, rows, cols, pad, dev, fill=float("nan"), dtype=None):
    """A rows x cols view of a rows x (cols + pad) float32 tensor (leading dimension cols + pad)."""
    full = torch.full((rows, cols + pad), fill, dtype=dtype or torch.float32, device=dev)
    return full[:, :cols]


def test_rp_f32_world1_sweep(crp, orc, gpu):
    """Every width, both layouts, device and host operands, padded leading dimensions and the three fp32 variants,
    against the fp64 oracle on B rounded to fp32; device row-major operands bit-identical to crp_spmm_csr_f32."""
    import torch
    from crp_spmm_amd import comm, engine, hip
    sc = comm.SelfComm()
    for name, rp, ci, va, k in _cases():
        m = len(rp) - 1
        A = hip.CsrDev(m, k, rp, ci, va)
        for n in WIDTHS:
            eng = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
            B32 = np.random.default_rng(n).uniform(-1, 1, size=(k, n)).astype(np.float32)
            ref = orc.spmm_csr(rp, ci, va, B32.astype(np.float64))
            Bd = torch.from_numpy(B32).to(gpu)
            Bd_pad = _padded(torch, k, n, 5, gpu)
            Bd_pad.copy_(Bd)
            Bcm_pad = _padded(torch, n, k, 3, gpu)                   # column-major k x n, ld k + 3
            Bcm_pad.copy_(Bd.t())
            for variant in (0, 1, 5):
                eng.set_variant_f32(variant)
                tag = (name, n, variant)
                # device, row-major, ld = n: bit-identical to the device-level product at the same variant
                Cd = torch.full((m, n), float("nan"), dtype=torch.float32, device=gpu)
                eng.exec(0, Bd, Cd)
                Cx = torch.full((m, n), float("nan"), dtype=torch.float32, device=gpu)
                hip.spmm_csr_f32(A, Bd, Cx, n=n, variant=variant)
                torch.cuda.synchronize()
                got = Cd.cpu().numpy()
                assert orc.rel_fro_err(ref, got.astype(np.float64)) <= FP32_TOL, tag
                assert np.array_equal(_bits(got), _bits(Cx.cpu().numpy())), tag + ("not bit-identical to crp_spmm_csr_f32",)
                # device, row-major, ldB = n + 5, ldC = n + 2
                Cp = _padded(torch, m, n, 2, gpu)
                eng.exec(0, Bd_pad, Cp)
                torch.cuda.synchronize()
                assert orc.rel_fro_err(ref, Cp.cpu().numpy().astype(np.float64)) <= FP32_TOL, tag + ("rm padded",)
                # device, column-major (operands as (n, ld) tensors), ldB = k + 3, ldC = m + 1
                Ccm = _padded(torch, n, m, 1, gpu)
                eng.exec(1, Bcm_pad, Ccm)
                torch.cuda.synchronize()
                assert orc.rel_fro_err(ref, Ccm.cpu().numpy().T.astype(np.float64)) <= FP32_TOL, tag + ("cm device",)
                # host (numpy) operands, both layouts, padded
                Bh = np.full((k, n + 3), np.nan, np.float32)
                Bh[:, :n] = B32
                Ch = np.full((m, n + 1), np.nan, np.float32)
                eng.exec(0, Bh[:, :n], Ch[:, :n])
                assert orc.rel_fro_err(ref, Ch[:, :n].astype(np.float64)) <= FP32_TOL, tag + ("rm host",)
                assert np.isnan(Ch[:, n]).all(), tag + ("host C padding written",)
                Bhc = np.full((n, k + 2), np.nan, np.float32)
                Bhc[:, :k] = B32.T
                Chc = np.full((n, m + 3), np.nan, np.float32)
                eng.exec(1, Bhc[:, :k], Chc[:, :m])
                assert orc.rel_fro_err(ref, Chc[:, :m].T.astype(np.float64)) <= FP32_TOL, tag + ("cm host",)
                assert np.isnan(Chc[:, m:]).all(), tag + ("host C padding written",)
            eng.free()
        A.free()
    sc.free()


def test_rp_f32_values_and_interleaving(crp, orc, gpu):
    """update_values reaches the fp32 exec; fp64 execs around an fp32 one are unchanged bit for bit; an engine whose
    first exec is fp32 still runs fp64 at the fp64 bar."""
    import torch
    from crp_spmm_amd import comm, engine
    sc = comm.SelfComm()
    for name, rp, ci, va, k in _cases():
        m = len(rp) - 1
        n = 64
        B = np.random.default_rng(3).uniform(-1, 1, size=(k, n))
        B32 = B.astype(np.float32)
        Bd, Bd32 = torch.from_numpy(B).to(gpu), torch.from_numpy(B32).to(gpu)
        C64 = torch.empty((m, n), dtype=torch.float64, device=gpu)
        C32 = torch.empty((m, n), dtype=torch.float32, device=gpu)
        # fp64 -> fp32 -> fp64 on one engine, timing off (asynchronous returns)
        eng = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
        eng.set_timing(False)
        eng.exec(0, Bd, C64)
        torch.cuda.synchronize()
        first = C64.cpu().numpy().copy()
        assert orc.rel_fro_err(orc.spmm_csr(rp, ci, va, B), first) <= FP64_TOL, name
        eng.exec(0, Bd32, C32)
        C64.fill_(float("nan"))
        eng.exec(0, Bd, C64)
        torch.cuda.synchronize()
        assert np.array_equal(C64.cpu().numpy(), first), (name, "fp64 after fp32 differs")
        assert orc.rel_fro_err(orc.spmm_csr(rp, ci, va, B32.astype(np.float64)),
                               C32.cpu().numpy().astype(np.float64)) <= FP32_TOL, name
        # update_values right after an asynchronous fp32 exec, then fp32 again: the new product
        va2 = 0.5 * va - 1.0
        eng.exec(0, Bd32, C32)
        eng.update_values(va2)
        C32.fill_(float("nan"))
        eng.exec(0, Bd32, C32)
        torch.cuda.synchronize()
        assert orc.rel_fro_err(orc.spmm_csr(rp, ci, va2, B32.astype(np.float64)),
                               C32.cpu().numpy().astype(np.float64)) <= FP32_TOL, (name, "update_values")
        eng.free()
        # first exec fp32, then fp64
        eng = engine.RpSpmm(0, m, rp, ci, va, [0, k], n, sc)
        eng.exec(0, Bd32, C32)
        eng.exec(0, Bd, C64)
        torch.cuda.synchronize()
        assert orc.rel_fro_err(orc.spmm_csr(rp, ci, va, B), C64.cpu().numpy()) <= FP64_TOL, (name, "fp64 after first fp32")
        eng.free()
    sc.free()


def test_para2d_f32_world1(crp, orc, gpu):
    """The 2D engine's fp32 exec on a 1 x 1 grid forwards to the row engine."""
    import torch
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.fem3d(8)
    m = len(rp) - 1
    sc = comm.SelfComm()
    for n in (30, 128):
        B32 = np.random.default_rng(n).uniform(-1, 1, size=(m, n)).astype(np.float32)
        ref = orc.spmm_csr(rp, ci, va, B32.astype(np.float64))
        e2 = engine.Para2dSpmm(sc, 1, 1, [0, m], [0, m], [0, m], [0, n], rp, ci, va)
        Cd = torch.full((m, n), float("nan"), dtype=torch.float32, device=gpu)
        e2.exec(0, torch.from_numpy(B32).to(gpu), Cd)
        torch.cuda.synchronize()
        assert orc.rel_fro_err(ref, Cd.cpu().numpy().astype(np.float64)) <= FP32_TOL, n
        Ch = np.full((n, m), np.nan, np.float32)
        e2.exec(1, np.ascontiguousarray(B32.T), Ch)
        assert orc.rel_fro_err(ref, Ch.T.astype(np.float64)) <= FP32_TOL, n
        e2.free()
    sc.free()


@pytest.mark.parametrize("n", [1, 7, 30, 64, 257, 1024])
def test_row_kernels_f32_bit_exact(crp, gpu, n):
    """gather / scatter / transpose in fp32 against torch indexing and transposition, bit for bit (NaN payloads
    included): odd widths, padded leading dimensions, pointers 4, 8 and 16 bytes off a 16-byte boundary."""
    import torch
    from crp_spmm_amd import hip
    g = torch.Generator(device="cpu").manual_seed(n)
    nsrc, nidx = 301, 173
    ridx = torch.randperm(nsrc, generator=g)[:nidx].to(torch.int32).to(gpu)
    ridx_l = ridx.long()
    for off in (0, 1, 2, 4):
        for pad in (0, 3, 8):
            ld = n + off + pad
            tag = (n, off, pad)
            # row-major
            src_full = torch.randn((nsrc, ld), generator=g).to(gpu)
            src_full[::17, ::5] = float("nan")
            src = src_full[:, off:off + n]
            dst_full = torch.full((nidx, ld), -7.0, device=gpu)
            dst = dst_full[:, off:off + n]
            hip.gather_rows_f32(ridx, src, dst)
            torch.cuda.synchronize()
            assert torch.equal(dst.contiguous().view(torch.int32), src[ridx_l].contiguous().view(torch.int32)), tag
            assert (dst_full[:, :off] == -7.0).all() and (dst_full[:, off + n:] == -7.0).all(), tag
            out_full = torch.full((nsrc, ld), -7.0, device=gpu)
            out = out_full[:, off:off + n]
            hip.scatter_rows_f32(ridx, dst, out)
            torch.cuda.synchronize()
            want = torch.full((nsrc, ld), -7.0, device=gpu)
            want[:, off:off + n][ridx_l] = dst
            assert torch.equal(out_full.view(torch.int32), want.view(torch.int32)), tag
            # column-major: (n, ld) tensors, rows of the matrix along the fast dimension
            csrc_full = torch.randn((n, nsrc + off + pad), generator=g).to(gpu)
            csrc = csrc_full[:, off:off + nsrc]
            cdst_full = torch.full((n, nidx + off + pad), -7.0, device=gpu)
            cdst = cdst_full[:, off:off + nidx]
            hip.gather_rows_f32(ridx, csrc, cdst, layout=1)
            torch.cuda.synchronize()
            assert torch.equal(cdst.contiguous().view(torch.int32), csrc[:, ridx_l].contiguous().view(torch.int32)), tag
            cout_full = torch.full((n, nsrc + off + pad), -7.0, device=gpu)
            cout = cout_full[:, off:off + nsrc]
            hip.scatter_rows_f32(ridx, cdst, cout, layout=1)
            torch.cuda.synchronize()
            cwant = torch.full((n, nsrc + off + pad), -7.0, device=gpu)
            cwant[:, off:off + nsrc][:, ridx_l] = cdst
            assert torch.equal(cout_full.view(torch.int32), cwant.view(torch.int32)), tag
            # transpose: nsrc x n (ld) -> n x nsrc (ld nsrc + off + pad)
            tdst_full = torch.full((n, nsrc + off + pad), -7.0, device=gpu)
            tdst = tdst_full[:, off:off + nsrc]
            hip.transpose_f32(src, tdst)
            torch.cuda.synchronize()
            assert torch.equal(tdst.contiguous().view(torch.int32), src.t().contiguous().view(torch.int32)), tag
            assert (tdst_full[:, :off] == -7.0).all() and (tdst_full[:, off + nsrc:] == -7.0).all(), tag


@pytest.mark.parametrize("world", [2, 4])
def test_engines_f32_multi_rank_one_gpu(world):
    """World 2 / 4 on the one card, host-staged exchange (tests/gpu_dist_f32_worker.py)."""
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    env["CRPSPMM_EXCHANGE"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29740 + world),
           os.path.join(ROOT, "tests", "gpu_dist_f32_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_F32_WORKER_OK world=%d" % world in r.stdout
