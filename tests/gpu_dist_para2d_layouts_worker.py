"""Worker for tests/test_gpu_para2d_layouts.py and tests/test_dist_para2d_layouts_cpu.py: what the 2D (pm x pn) engine adds above
the row engine -- update_values, update_values_dev, exec_t, exec_t_f32 and sddmm -- on N ranks, on the grids no other test runs:
a rectangular A whose B blocks have nothing to do with its panels, slices whose runs of the panel are odd in length and start at
odd offsets, a slice of one row, an empty slice, a grid row without rows of A, a grid row without rows of B, and widths that leave
grid columns without a column of B.  Matrices, exact data and operand forms are those of tests/gpu_dist_layouts_worker.py: every
result has ONE correct bit pattern.

  (no argument)  on the GPU: N ranks sharing one card with the exchange staged through the host, or a GPU per rank and RCCL
  --plan-only    on the CPU over gloo: the slice bookkeeping, the value update and the SDDMM's data flow replayed in numpy
  --only=NAMES   (either half) only the matrices named, comma-separated: band, rect, lower

Both halves take their grids from grids() below."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gpu_dist_layouts_worker import T_FORMS, Data, Operands, bits, check_exact, check_sddmm, matrices, part_of  # noqa: E402

WIDTHS = (1, 7, 33)              # with pn > 1: some grid columns hold no column; slices of 2, 2, 2, 1 at pn = 4; odd and > 16
ROUNDED_N = 7                    # the width of the one rounded case per (matrix, grid)
DEV_FORM = ("dev", 0, 1, 1)      # the operand form of the forward product after a device update


def _i32(a):
    return np.asarray(a, dtype=np.int32)


def _balanced_slices(planner, rp, ac, pm, pn):
    """A0_rowptr: every panel cut into pn slices of balanced nonzero counts (a panel without rows: pn empty slices)."""
    a0 = np.zeros(pm * pn + 1, dtype=np.int32)
    for i in range(pm):
        lo, hi = int(ac[i]), int(ac[i + 1])
        a0[i * pn:(i + 1) * pn + 1] = planner.csr_mat_row_partition(rp[lo:hi + 1] - rp[lo], pn) + lo if hi > lo else lo
    return a0


def run_offsets(rp, a0, pm, pn):
    """(pm, pn + 1): where every slice of a grid row starts in its panel, in nonzeros."""
    return np.array([[int(rp[a0[i * pn + j]]) - int(rp[a0[i * pn]]) for j in range(pn + 1)] for i in range(pm)], dtype=np.int64)


def grids(planner, rp, m, k, P):
    """[(name, pm, pn, a0, br, ac)] for every pn that divides P: A0_rowptr (P + 1), B_rowptr (pm + 1), AC_rowptr (pm + 1).  The
    property every grid is there for is asserted here, so a change of a generator cannot quietly empty the test."""
    out = []
    for pn in [d for d in range(1, P + 1) if P % d == 0]:
        pm = P // pn
        ac = _i32(planner.csr_mat_row_partition(rp, pm) if m == k else planner.even_displs(m, pm))
        br = ac if m == k else _i32(planner.even_displs(k, pm))
        bal = _balanced_slices(planner, rp, ac, pm, pn)
        out.append(("bal", pm, pn, bal, br, ac))
        if m != k:
            assert not np.array_equal(br, ac), "rect: the B blocks and the panels must differ"
        if pn >= 2:
            # odd: every cut inside a panel moves to the first row at or after it where the panel's running count is odd
            a0 = bal.copy()
            for i in range(pm):
                lo, hi = int(ac[i]), int(ac[i + 1])
                for j in range(1, pn):
                    r = max(int(a0[i * pn + j]), int(a0[i * pn + j - 1]))
                    while r < hi and (int(rp[r]) - int(rp[lo])) % 2 == 0:
                        r += 1
                    a0[i * pn + j] = r
            off = run_offsets(rp, a0, pm, pn)
            for i in range(pm):
                lens = np.diff(off[i])
                assert (lens % 2 == 1).any(), ("odd", pm, pn, i, "no run of odd length")
                assert ((off[i, :pn] % 2 == 1) & (lens > 0)).any(), ("odd", pm, pn, i, "no run starts at an odd offset")
            out.append(("odd", pm, pn, a0, br, ac))
            # one: the first slice of grid row 0 ends with the first non-empty row
            a0 = bal.copy()
            a0[1] = int(np.flatnonzero(np.diff(rp) > 0)[0]) + 1
            first = int(rp[a0[1]] - rp[a0[0]])
            assert a0[1] <= a0[2] and 1 <= first <= 16 and first == int(np.diff(rp)[a0[1] - 1]), ("one", pm, pn, a0[:3], first)
            out.append(("one", pm, pn, a0, br, ac))
            # none: the first rank of grid row 0 holds no row of A0
            a0 = bal.copy()
            a0[0:2] = ac[0]
            assert rp[a0[1]] == rp[a0[0]] and rp[a0[2]] > rp[a0[1]], ("none", pm, pn)
            out.append(("none", pm, pn, a0, br, ac))
        if pm >= 2:
            # nopanel: grid row 1 owns no row of A -- every slice of it is empty
            e = planner.even_displs(m, pm - 1)
            ac1 = _i32(np.concatenate([e[:2], e[1:]]))
            a0 = _balanced_slices(planner, rp, ac1, pm, pn)
            assert ac1[1] == ac1[2] and (a0[pn:2 * pn + 1] == ac1[1]).all(), ("nopanel", pm, pn, ac1)
            out.append(("nopanel", pm, pn, a0, _i32(planner.even_displs(k, pm)), ac1))
            # noB: grid row 0 owns no row of B
            ac2 = _i32(planner.even_displs(m, pm))
            br2 = _i32(np.concatenate([[0], planner.even_displs(k, pm - 1)]))
            assert br2[0] == br2[1] == 0 and rp[ac2[1]] > rp[ac2[0]], ("noB", pm, pn, br2)
            out.append(("noB", pm, pn, _balanced_slices(planner, rp, ac2, pm, pn), br2, ac2))
    for name, pm, pn, a0, br, ac in out:
        t = (name, pm, pn, a0, br, ac)
        assert a0.size == P + 1 and br.size == ac.size == pm + 1 and a0[0] == br[0] == ac[0] == 0, t
        assert a0[P] == ac[pm] == m and br[pm] == k, t
        assert (np.diff(a0) >= 0).all() and (np.diff(br) >= 0).all() and (np.diff(ac) >= 0).all(), t
        assert all(a0[i * pn] == ac[i] for i in range(pm + 1)), t
    return out


def grids_of(planner, name, rp, m, k, P):
    """`lower` runs on grid `bal` alone."""
    return [g for g in grids(planner, rp, m, k, P) if name != "lower" or g[0] == "bal"]


def rounded_t(data, n):
    """{"f64" | "f32": (val in A's order, B (m x n), (ref, bound) of C = A^T B (k x n))}: ordinary rounded data generated on the
    TRANSPOSED pattern, the values carried back to A's order as Data.exact_t_sets does; ref and bound are fp64_ref.f64_bound /
    fp32_ref.f32_bound of the transposed CSR, (L_c + 1) u (|A^T| |B|) with L_c the nonzeros of A's column c."""
    import fp32_ref
    import fp64_ref

    def make():
        rp_t, ci_t, order = data.transposed()
        val_t, B = fp64_ref.rounded_problem(rp_t, ci_t, data.m, n, np.random.default_rng(data.seed + 1000 * n + 19))
        val = np.empty_like(val_t)
        val[order] = val_t
        rng = np.random.default_rng(data.seed + 1000 * n + 23)
        v32, B32 = fp32_ref.data_values(rng, int(data.rp[-1])), fp32_ref.data_B(rng, (data.m, n))
        return {"f64": (val, B, fp64_ref.f64_bound(rp_t, ci_t, val_t, B)), "f32": (v32, B32, fp32_ref.f32_bound(rp_t, ci_t, v32[order], B32))}
    return data._get(("rt", n), make)


# ---------------------------------------------------------------------------------------------------------------- CPU half
def plan_only_main():
    import torch.distributed as dist
    from crp_spmm_amd import comm as crp_comm, engine, gen, planner
    from dist_para2d_ops_worker import partial_dots, reduce_scatter

    crp_comm.init_process_group()
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    controls = 0
    for name, rp, ci, m, k in matrices(gen):
        data = Data(name, rp, ci, m, k)
        for gname, pm, pn, a0, br, ac in grids_of(planner, name, rp, m, k, P):
            pi, pj = me // pn, me % pn
            mine = slice(int(rp[a0[me]]), int(rp[a0[me + 1]]))
            panel = slice(int(rp[ac[pi]]), int(rp[ac[pi + 1]]))
            for n in WIDTHS:
                tag = (me, name, gname, "%dx%d" % (pm, pn), n)
                bc = planner.even_displs(n, pn)
                c0, c1 = int(bc[pj]), int(bc[pj + 1])
                val, X, Y, out0, out1 = data.sddmm_set(n)
                first = data.exact64(n, "A").val
                e2 = engine.Para2dSpmm(world, pm, pn, a0, br, ac, bc, *part_of(rp, ci, first, a0, me), plan_only=True)
                col_comm = None
                for c in list(crp_comm._live.values()):
                    if c.nproc == pm and c is not world and c.rank == pi:
                        col_comm = c                             # (the grid-row communicator of init is gone by now)
                assert col_comm is not None, tag
                # ---- the slice counts against A0_rowptr
                want_row = np.array([rp[a0[pi * pn + j + 1]] - rp[a0[pi * pn + j]] for j in range(pn)], np.int64)
                assert np.array_equal(e2.row_slice_nnz, want_row) and e2.slice_nnz == mine.stop - mine.start == int(want_row[pj]), tag
                assert np.array_equal(e2.rp.plan()["A_val"], first[panel]), tag + ("init",)
                # ---- a second value set reaches the inner plan as the grid row's slices concatenated in rank order
                before = set(crp_comm._live)
                e2.update_values(val[mine])
                plan = e2.rp.plan()
                assert np.array_equal(plan["A_val"], val[panel]), tag + ("update_values",)
                fresh = [c for a, c in crp_comm._live.items() if a not in before]
                assert len(fresh) == (1 if pn > 1 else 0), tag
                # ---- the SDDMM's data flow: partial dots over this rank's columns in panel order, the runs moved along the grid row
                #      by row_slice_nnz, summed in ascending grid column -- every number exact, so `out` has one bit pattern
                X_loc = np.ascontiguousarray(X[ac[pi]:ac[pi + 1], c0:c1])
                Y_loc = np.ascontiguousarray(Y[br[pi]:br[pi + 1], c0:c1])
                for mode, want in ((0, out0[mine]), (1, out1[mine])):
                    part = partial_dots(plan, col_comm if pm > 1 else None, X_loc, Y_loc, c1 - c0, mode)
                    assert part.size == panel.stop - panel.start, tag
                    got = reduce_scatter(fresh[0], part, want_row, pj) if pn > 1 else part
                    assert got.shape == want.shape and np.array_equal(got, want), tag + (mode, "emulated sddmm")
                    if gname == "odd" and n == WIDTHS[-1]:
                        # negative control: every run read from its start rounded DOWN to an even index -- the mistake the fp32 send
                        # slots exist to prevent -- must not give the expected `out` on the ranks whose run starts at an odd offset
                        off = np.concatenate([[0], np.cumsum(want_row)])[:pn]
                        wrong = reduce_scatter(fresh[0], part, want_row, pj, starts=off // 2 * 2)
                        if off[pj] % 2 == 1 and want_row[pj] > 0:
                            assert not np.array_equal(wrong, want), tag + (mode, "the data does not see a run read one entry early")
                            controls += 1
                        else:
                            assert np.array_equal(wrong, want), tag + (mode, "a run that starts on a word moved")
                e2.free()
            dist.barrier()
    import torch
    seen = torch.tensor([controls])
    dist.all_reduce(seen)
    assert int(seen) > 0, "the negative control ran on no rank"
    if me == 0:
        print("DIST_PARA2D_LAYOUTS_PLAN_OK world=%d controls=%d" % (P, int(seen)))
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------- GPU half
class _Timed:
    """What check_sddmm calls on an engine: Para2dSpmm keeps set_timing on its row engine."""

    def __init__(self, e2):
        self.sddmm, self.set_timing = e2.sddmm, e2.rp.set_timing


def gpu_main():
    import torch
    import torch.distributed as dist
    import fp32_ref
    import fp64_ref
    from crp_spmm_amd import comm as crp_comm, engine, gen, planner

    native = os.environ.get("CRPSPMM_EXPECT_NATIVE_RCCL") == "1"
    idev = int(os.environ.get("LOCAL_RANK", "0")) if native else 0
    torch.cuda.set_device(idev)
    dev = torch.device("cuda", idev)
    crp_comm.init_process_group(device=idev if native else None)
    assert crp_comm.exchange_mode() == ("nccl" if native else "host")
    world = crp_comm.TorchComm()
    if native:
        assert world.device_ranks() == world.nproc, "the native RCCL communicator did not come up"
    P, me = world.nproc, world.rank

    def dev_vals(v, dt):
        """The slice's values as update_values_dev takes them: an empty slice passes an empty tensor, whose pointer is NULL."""
        if v.size == 0:
            t = torch.empty(0, dtype=dt, device=dev)
            assert t.data_ptr() == 0
            return t
        assert dt == torch.float64 or np.array_equal(v.astype(np.float32).astype(np.float64), v), "not fp32-representable"
        return torch.from_numpy(np.ascontiguousarray(v)).to(device=dev, dtype=dt)

    def put(e2, route, v):
        """One set of slice values by its route: 0 the host update, 1 a float64 device tensor, 2 a float32 device tensor."""
        if route == 0:
            e2.update_values(v)
        else:
            e2.update_values_dev(dev_vals(v, torch.float64 if route == 1 else torch.float32))

    for name, rp, ci, m, k in matrices(gen):
        data = Data(name, rp, ci, m, k)
        rp_t = data.transposed()[0]
        for gname, pm, pn, a0, br, ac in grids_of(planner, name, rp, m, k, P):
            pi, pj = me // pn, me % pn
            r0, r1, b0, b1 = int(ac[pi]), int(ac[pi + 1]), int(br[pi]), int(br[pi + 1])
            mine = slice(int(rp[a0[me]]), int(rp[a0[me + 1]]))
            panel = slice(int(rp[r0]), int(rp[r1]))
            for n in WIDTHS:
                bc = planner.even_displs(n, pn)
                c0, c1 = int(bc[pj]), int(bc[pj + 1])
                tag = (me, name, gname, "%dx%d" % (pm, pn), n)
                blk = lambda M, lo, hi: np.ascontiguousarray(M[lo:hi, c0:c1])
                t_sets = data.exact_t_sets(n)
                e2 = engine.Para2dSpmm(world, pm, pn, a0, br, ac, bc, *part_of(rp, ci, data.exact64(n, "A").val, a0, me))
                assert e2.slice_nnz == mine.stop - mine.start and not e2.sddmm_built, tag
                # ---- 1. exec_t / exec_t_f32: the rank's block of C = A^T B bit for bit; the three value sets by the three routes;
                #      every operand form with timing on once and off once
                for route, (what, val, B, C_exact) in enumerate(t_sets):
                    put(e2, route, val[mine])
                    call = e2.exec_t_f32 if B.dtype == np.float32 else e2.exec_t
                    for form in T_FORMS:
                        check_exact(torch, dev, call, e2.rp.set_timing, form, blk(B, r0, r1), blk(C_exact, b0, b1), b1 - b0, c1 - c0,
                                    tag + (what,), reps=1)
                assert e2.rp.host_values_stale == (panel.stop > panel.start), tag
                assert np.array_equal(bits(e2.rp.plan()["A_val"]), bits(t_sets[2][1][panel])), tag + ("the panel's values after update_values_dev",)
                assert not e2.rp.host_values_stale, tag
                # ---- 2. sddmm: `out` over the rank's own slice bit for bit, both dtypes, both modes; the NULL Y where a grid row has no
                #      rows of B (every rank runs that form then: each call is an exchange all ranks take part in)
                val, X, Y, out0, out1 = data.sddmm_set(n)
                e2.update_values(val[mine])
                sd_forms = T_FORMS + ((("dev", 0, 0, 0),) if (np.diff(br) == 0).any() else ())
                for dt in (np.float64, np.float32):
                    for form in sd_forms:
                        check_sddmm(torch, dev, _Timed(e2), form, blk(X, r0, r1).astype(dt), blk(Y, b0, b1).astype(dt),
                                    (out0[mine].astype(dt), out1[mine].astype(dt)), tag + ("sddmm", np.dtype(dt).name))
                assert e2.sddmm_built == (pn > 1), tag
                # ---- 3. the forward product after a device update, against a product whose bits are known
                for route, (what, val, B, C_exact) in enumerate(data.exact_sets(n)):
                    put(e2, route, val[mine])
                    check_exact(torch, dev, e2.exec, e2.rp.set_timing, DEV_FORM, blk(B, b0, b1), blk(C_exact, r0, r1), r1 - r0, c1 - c0,
                                tag + (what, "route %d" % route), reps=1)
                # ---- 4. one rounded case per matrix and grid: every entry of the rank's block within the derived bound of A^T B
                if n == ROUNDED_N:
                    for key, call, check in (("f64", e2.exec_t, fp64_ref.check_f64_bound), ("f32", e2.exec_t_f32, fp32_ref.check_f32_bound)):
                        val, B, (ref, bound) = rounded_t(data, n)[key]
                        e2.update_values(val[mine])
                        ops = Operands(torch, dev, DEV_FORM, blk(B, r0, r1), b1 - b0, c1 - c0)
                        ops.reset_c()
                        call(0, ops.B, ops.C)
                        check(rp_t[b0:b1 + 1], None, None, None, ops.result(tag + ("rounded", key)),
                              what="rank %d %s %s %dx%d n=%d rounded %s exec_t" % (me, name, gname, pm, pn, n, key),
                              ref_bound=(ref[b0:b1, c0:c1], bound[b0:b1, c0:c1]))
                e2.free()
            dist.barrier()
    if me == 0:
        print("GPU_DIST_PARA2D_LAYOUTS_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    if "--plan-only" in sys.argv[1:]:
        plan_only_main()
    else:
        gpu_main()
