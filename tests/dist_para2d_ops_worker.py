"""Worker for tests/test_para2d_ops.py: one process per rank, gloo backend, CPU only.  Every pm x pn grid of the world gets a
plan-only 2D engine; checked are the slice counts the engine keeps (slice_nnz / row_slice_nnz), the value update (the grid
row's slice values all-gathered into panel order) and -- replayed in numpy -- the data flow of the 2D SDDMM: partial dots
over the rank's column slice in panel order from the inner plan, the runs moved along the grid row by row_slice_nnz, and
the pn runs summed in ascending grid column, against the global SDDMM in the order of the rank's own slice."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPLAY_TOL = 1e-13          # relative; the tolerance of the replays in tests/dist_worker.py


def slices(rp, ci, va, displs, r):
    s, e = displs[r], displs[r + 1]
    return rp[s:e + 1], ci[rp[s]:rp[e]], va[rp[s]:rp[e]]


def _ll(a):
    return np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_longlong))


def partial_dots(plan, col_comm, X_loc, Y_loc, n_loc, mode):
    """The inner engine's SDDMM over n_loc columns (the replay of tests/dist_sddmm_worker.py): one value per panel nonzero.  A rank
    whose panel has no nonzeros still serves the exchange; a block without rows or without columns (n_loc == 0) gives zeros."""
    nnz = plan["A_colidx"].size
    code = plan["dev_colidx"].astype(np.int64)
    rows = np.repeat(np.arange(plan["A_nrow"]), np.diff(plan["A_rowptr"]))
    Y1 = np.zeros((0, n_loc))
    if col_comm is None:                                         # one grid row: every column of the panel is local
        assert (code >= 0).all()
    else:
        P = plan["nproc"]
        send = np.ascontiguousarray(Y_loc[plan["rB_sridxs"], :n_loc]).reshape(-1)
        if send.size == 0:
            send = np.zeros(1)
        nrecv = int(plan["rB_rdispls"][P])
        recv = np.full(max(nrecv, 1), np.nan)
        sc, sd, rc, rd = (np.ascontiguousarray(plan[k], dtype=np.int64) for k in ("rB_scnts", "rB_sdispls", "rB_rcnts", "rB_rdispls"))
        col_comm.struct.alltoallv_dev_f64(None, send.ctypes.data, _ll(sc), _ll(sd), recv.ctypes.data, _ll(rc), _ll(rd), None)
        Y1 = recv[:nrecv].reshape(nrecv // n_loc if n_loc else 0, n_loc)
    if nnz == 0:
        return np.zeros(0)
    loc = code >= 0
    yrows = np.zeros((nnz, n_loc))
    yrows[loc] = Y_loc[code[loc]]
    yrows[~loc] = Y1[~code[~loc]]
    out = np.einsum("ij,ij->i", X_loc[rows], yrows)
    return out * plan["A_val"] if mode else out


def reduce_scatter(row_comm, part, row_nnz, pj, starts=None):
    """Peer j is sent the run [off_j, off_j + nnz_j) of `part`; this rank receives pn runs of its own slice, added in
    ascending grid column.  starts: where the runs are read from instead of off (a negative control's wrong offsets)."""
    pn = row_nnz.size
    off = np.concatenate([[0], np.cumsum(row_nnz)]).astype(np.int64)
    mine = int(row_nnz[pj])
    recv = np.full(max(pn * mine, 1), np.nan)
    send = part if part.size else np.zeros(1)
    sc, sd = row_nnz.astype(np.int64), (off[:pn].copy() if starts is None else np.ascontiguousarray(starts, dtype=np.int64))
    rc, rd = np.full(pn, mine, np.int64), np.arange(pn, dtype=np.int64) * mine
    row_comm.struct.alltoallv_dev_f64(None, send.ctypes.data, _ll(sc), _ll(sd), recv.ctypes.data, _ll(rc), _ll(rd), None)
    seg = recv[:pn * mine].reshape(pn, mine)
    out = seg[0].copy()
    for j in range(1, pn):
        out = out + seg[j]
    return out


def check_grid(world, crp_comm, engine, pm, pn, a0, ac, bc, rp, ci, va, X, Y, tag):
    import torch.distributed as dist
    P, me = world.nproc, world.rank
    pi, pj = me // pn, me % pn
    my = slices(rp, ci, va, a0, me)
    e2 = engine.Para2dSpmm(world, pm, pn, a0, ac, ac, bc, *my, plan_only=True)
    col_comm = None
    for c in list(crp_comm._live.values()):
        if c.nproc == pm and c is not world and c.rank == pi:
            col_comm = c                                         # (the grid-row communicator of init is gone by now)
    assert col_comm is not None, (me, tag)
    # (a) the slice counts of the grid row
    want_row = np.array([rp[a0[pi * pn + j + 1]] - rp[a0[pi * pn + j]] for j in range(pn)], np.int64)
    got_row = e2.row_slice_nnz
    assert got_row.dtype == np.int64 and np.array_equal(got_row, want_row), (me, tag, got_row, want_row)
    assert e2.slice_nnz == my[2].size == int(want_row[pj]), (me, tag)
    assert not e2.sddmm_built
    # (b) the value update reaches the inner plan in panel order
    before = set(crp_comm._live)
    e2.update_values(3.0 * my[2] + 1.0)
    ps, pe = int(rp[ac[pi]]), int(rp[ac[pi + 1]])
    plan = e2.rp.plan()
    assert np.array_equal(plan["A_val"], 3.0 * va[ps:pe] + 1.0), (me, tag, "update_values")
    fresh = [c for a, c in crp_comm._live.items() if a not in before]
    assert len(fresh) == (1 if pn > 1 else 0), (me, tag, "the grid-row communicator is split by the first update, once")
    e2.update_values(3.0 * my[2] + 1.0)
    assert set(crp_comm._live) == before | {C.addressof(c.struct) for c in fresh}, (me, tag, "and kept")
    with np.testing.assert_raises(ValueError):
        e2.update_values(np.zeros(my[2].size + 1))
    # the data flow of sddmm, replayed
    n_loc = int(bc[pj + 1] - bc[pj])
    X_loc = np.ascontiguousarray(X[ac[pi]:ac[pi + 1], bc[pj]:bc[pj + 1]])
    Y_loc = np.ascontiguousarray(Y[ac[pi]:ac[pi + 1], bc[pj]:bc[pj + 1]])
    grow = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    s0, s1 = int(rp[a0[me]]), int(rp[a0[me + 1]])
    for mode in (0, 1):
        part = partial_dots(plan, col_comm if pm > 1 else None, X_loc, Y_loc, n_loc, mode)
        assert part.size == pe - ps
        got = reduce_scatter(fresh[0], part, want_row, pj) if pn > 1 else part
        ref = np.einsum("ij,ij->i", X[grow[s0:s1]], Y[ci[s0:s1]]) * ((3.0 * va[s0:s1] + 1.0) if mode else 1.0)
        assert got.shape == ref.shape, (me, tag, mode)
        assert np.linalg.norm(got - ref) <= REPLAY_TOL * np.linalg.norm(ref), (me, tag, mode, np.linalg.norm(got - ref))
    e2.free()
    dist.barrier()


def main():
    import torch.distributed as dist
    from crp_spmm_amd import comm as crp_comm, engine, gen, planner

    crp_comm.init_process_group()
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    m = k = 900
    n = 12
    rp, ci, va = gen.banded_fem(m, offsets=(1, 2, 3, 40, 41, 300), seed=9)
    rng = np.random.default_rng(17)
    X, Y = rng.standard_normal((m, n)), rng.standard_normal((k, n))
    rb = planner.csr_mat_row_partition(rp, P)
    for pn in [d for d in range(1, P + 1) if P % d == 0]:
        pm = P // pn
        ac = np.array([rb[i * pn] for i in range(pm + 1)], dtype=np.int32)
        a0 = np.zeros(P + 1, dtype=np.int32)
        for i in range(pm):
            loc = rp[ac[i]:ac[i + 1] + 1] - rp[ac[i]]
            a0[i * pn:(i + 1) * pn + 1] = planner.csr_mat_row_partition(loc, pn) + ac[i]
        bc = planner.even_displs(n, pn)
        check_grid(world, crp_comm, engine, pm, pn, a0, ac, bc, rp, ci, va, X, Y, "%dx%d" % (pm, pn))
    # (c) a grid row whose first rank holds no rows of A0: pm x 2, A0_rowptr by hand
    pn, pm = 2, P // 2
    ac = np.array([m * i // pm for i in range(pm + 1)], dtype=np.int32)
    a0 = np.zeros(P + 1, dtype=np.int32)
    for i in range(pm):
        a0[2 * i], a0[2 * i + 1] = ac[i], (ac[i] + ac[i + 1]) // 2
    a0[0:2] = ac[0]                                               # rank 0: an empty slice
    a0[P] = m
    check_grid(world, crp_comm, engine, pm, pn, a0, ac, planner.even_displs(n, pn), rp, ci, va, X, Y, "%dx2 empty slice" % pm)
    if me == 0:
        print("DIST_PARA2D_OPS_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
