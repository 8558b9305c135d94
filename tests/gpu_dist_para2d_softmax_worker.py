"""Worker for tests/test_gpu_row_softmax.py: the 2D engine's row softmax over this rank's A0 slice on every pm x pn grid of N
ranks (2 ranks: 1 x 2, 2 x 1; 4 ranks: 1 x 4, 2 x 2, 4 x 1) -- sharing ONE GPU with device payloads staged through the host, or
with a GPU per rank and the native RCCL exchange.  The grid rows are cut by hand: a slice of one row, an empty slice, slices
that start at odd panel offsets.  Every rank forms the FULL matrix's result with the device-level call and asserts that its
engine's result is that array's slice bit for bit; after update_values_dev(y) on the grid, exec equals the run of a twin engine
after the host update_values with the downloaded y."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cut_rows(r0, r1, pn, variant):
    """pn + 1 row offsets of the slices of the panel [r0, r1): variant 0 -- a slice of one row first, then (pn >= 3) an empty
    one, the rest even; variant 1 -- an empty slice first, then one of an odd number of rows"""
    if pn == 1:
        return [r0, r1]
    head = [r0, r0 + 1] + ([r0 + 1] if pn >= 3 else []) if variant == 0 else [r0, r0, r0 + 37][:pn]
    rest = pn + 1 - len(head)
    return head + [head[-1] + (r1 - head[-1]) * (j + 1) // rest for j in range(rest)]


def run_grid(ctx, pm, pn, variant, mat, tag):
    import torch
    import torch.distributed as dist
    R, engine, hip, planner, world, dev = ctx
    rp, ci, va = mat
    m, n = rp.size - 1, 8
    P, me = world.nproc, world.rank
    pi, pj = me // pn, me % pn
    ac = np.array([m * i // pm for i in range(pm + 1)], dtype=np.int32)
    a0 = np.zeros(P + 1, dtype=np.int32)
    for i in range(pm):
        a0[i * pn:(i + 1) * pn + 1] = cut_rows(int(ac[i]), int(ac[i + 1]), pn, variant)
    assert a0[P] == m and (np.diff(a0) >= 0).all()
    bc = planner.even_displs(n, pn)
    c0, c1 = int(bc[pj]), int(bc[pj + 1])
    r0, r1 = int(ac[pi]), int(ac[pi + 1])
    mine = slice(int(rp[a0[me]]), int(rp[a0[me + 1]]))
    snz = mine.stop - mine.start
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # what the grid holds: cut 0 a slice of one row and a slice at an odd offset of its panel (pn >= 3: an empty one too),
    # cut 1 an empty slice first
    rows, p_off = int(a0[me + 1] - a0[me]), mine.start - int(rp[ac[pi]])
    flags = torch.tensor([int(rows == 1), int(rows == 0), int(p_off % 2 == 1 and snz > 0)], device=dev)
    dist.all_reduce(flags)
    if pn > 1 and variant == 0:
        assert int(flags[0]) > 0 and int(flags[2]) > 0 and (pn < 3 or int(flags[1]) > 0), (tag, flags.tolist())
    if pn > 1 and variant == 1:
        assert int(flags[1]) > 0, (tag, flags.tolist())

    mk = lambda: engine.Para2dSpmm(world, pm, pn, a0, ac, ac, bc, rp[a0[me]:a0[me + 1] + 1], ci[mine], va[mine])
    e2, twin = mk(), mk()
    assert e2.slice_nnz == snz and not e2.row_softmax_built, (me, tag)
    B = np.random.default_rng(51).uniform(-1, 1, (m, n))
    for ndt in (np.float64, np.float32):
        s = R.scores(rp, ndt, 8, 41)
        dy = R.grads(s.size, ndt, 42)
        rp_d, s_d, dy_d = T(rp), T(s), T(dy)
        full = hip.row_softmax(rp_d, s_d)
        full_b = hip.row_softmax_bwd(rp_d, full, dy_d)
        torch.cuda.synchronize()
        want, want_b = full.cpu().numpy()[mine], full_b.cpu().numpy()[mine]
        y = torch.full((snz,), float("nan"), dtype=s_d.dtype, device=dev)
        assert e2.row_softmax(s_d[mine].clone(), out=y) is y
        torch.cuda.synchronize()
        assert e2.row_softmax_built == (snz > 0), (me, tag)                  # an empty slice uploads nothing
        assert not e2.sddmm_built, (me, tag)                                 # (no grid-row buffers, no grid-row communicator)
        assert np.array_equal(y.cpu().numpy(), want), (me, tag, ndt.__name__, "forward")
        got = e2.row_softmax_bwd(y, dy_d[mine].clone())
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want_b), (me, tag, ndt.__name__, "backward")
        # the values go back into the engine without leaving HBM; the twin takes them through the host
        e2.update_values_dev(y)
        twin.update_values(want.astype(np.float64))
        Bd = T(B[r0:r1, c0:c1].astype(ndt))
        Ca, Cb = (torch.full((r1 - r0, c1 - c0), float("nan"), dtype=s_d.dtype, device=dev) for _ in range(2))
        e2.exec(0, Bd, Ca)
        twin.exec(0, Bd, Cb)
        torch.cuda.synchronize()
        ca = Ca.cpu().numpy()
        assert not np.isnan(ca).any() and np.array_equal(ca, Cb.cpu().numpy()), (me, tag, ndt.__name__, "exec after the update")
    e2.free()
    twin.free()
    dist.barrier()


def main():
    import torch
    import torch.distributed as dist
    import softmax_ref as R
    from crp_spmm_amd import comm as crp_comm, engine, gen, hip, planner

    native = os.environ.get("CRPSPMM_EXPECT_NATIVE_RCCL") == "1"
    idev = int(os.environ.get("LOCAL_RANK", "0")) if native else 0
    torch.cuda.set_device(idev)
    dev = torch.device("cuda", idev)
    crp_comm.init_process_group(device=idev if native else None)
    assert crp_comm.exchange_mode() == ("nccl" if native else "host")
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    ctx = (R, engine, hip, planner, world, dev)
    m = 2400
    rp, ci, va = gen.random_csr(m, m, 15)
    rp = rp.astype(np.int32)
    assert (np.diff(rp) % 2 == 1).any()
    for pn in [d for d in range(1, P + 1) if P % d == 0]:
        for variant in (0, 1) if pn > 1 else (0,):
            run_grid(ctx, P // pn, pn, variant, (rp, ci, va), "%dx%d cut %d" % (P // pn, pn, variant))
    if me == 0:
        print("GPU_DIST_PARA2D_SOFTMAX_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
