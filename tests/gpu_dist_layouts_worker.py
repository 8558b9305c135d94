"""Worker for tests/test_gpu_engine_layouts.py and tests/test_dist_layouts_cpu.py: the forward exec of the row-parallel and 2D
engines on N ranks, on the rank layouts no other test runs -- a rank without rows of A, a rank without rows of B, a rank that
sends but receives nothing, a rectangular A whose B partition has nothing to do with its row partition -- with odd widths and
padded, misaligned operands, on data whose product has ONE correct bit pattern (fp64_ref.exact_parts, fp32_ref.exact_problem32).
On the partitions with a rank that owns no row of A or of B (b, c, d) the row-parallel engine's transposed product and SDDMM run
too, at two widths, on exact data of their own (Data.exact_t_sets, Data.sddmm_set).

  (no argument)  on the GPU: N ranks sharing one card with the exchange staged through the host, or a GPU per rank and RCCL
  --plan-only    on the CPU over gloo: plan() against oracle.rp_plan_all and the emulated product of tests/dist_worker.py
  --only=NAMES   (either half) only the matrices named, comma-separated: band, rect, lower

Both halves take their matrices, partitions and data from the functions below, so the layouts are checked without a GPU too."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WIDTHS = (1, 7, 24, 33)          # scalar path; odd; a multiple of 4; odd and two 16-column pieces (fp32 ld32 != n for 1, 7, 33)
SENT = -7.0                      # what every element around an operand holds
T_WIDTHS = (7, 33)               # exec_t and sddmm: the widths ...
T_LAYOUTS = ("b", "c", "d")      # ... the partitions ...
T_FORMS = (("dev", 0, 1, 1), ("dev", 1, 3, 0), ("host", 1, 3, 0))        # ... and the operand forms they run on


def matrices(gen):
    """[(name, rowptr, colidx, m, k)]: identical on every rank."""
    rp, ci, _va = gen.banded_fem(1600, offsets=(1, 2, 3, 40))
    rows = np.repeat(np.arange(1600), np.diff(rp))
    keep = ci <= rows                                   # `lower`: rank 0 needs nothing from a peer, the last rank owes nothing
    rp_l = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=1600))]).astype(np.int32)
    rp_r, ci_r, _va = gen.random_csr(900, 700, 12, empty_every=7)
    mats = [("band", rp, ci, 1600, 1600), ("rect", rp_r, ci_r, 900, 700), ("lower", rp_l, ci[keep].astype(np.int32), 1600, 1600)]
    only = [a[len("--only="):].split(",") for a in sys.argv[1:] if a.startswith("--only=")]
    return [x for x in mats if not only or x[0] in only[0]]


def partitions(planner, rp, m, k, P):
    """[(letter, ra, rb)]: A's row displacements and B's, P + 1 entries each."""
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    ea, eb = i32(planner.even_displs(m, P)), i32(planner.even_displs(k, P))
    out = []
    if m == k:
        nb = i32(planner.csr_mat_row_partition(rp, P))
        out.append(("a", nb, nb))
    out.append(("b", ea, i32(np.concatenate([[0], planner.even_displs(k, P - 1)]))))            # rank 0 owns no row of B
    e1 = planner.even_displs(m, P - 1)
    out.append(("c", i32(np.concatenate([e1[:2], e1[1:]])), eb))                                 # rank 1 owns no row of A
    out.append(("d", ea, i32([0] * P + [k])))                                                    # the last rank owns all of B
    if m != k:
        out.append(("e", ea, eb))                                                                # two unrelated partitions
    for letter, ra, rb in out:
        assert ra.size == rb.size == P + 1 and ra[0] == rb[0] == 0 and ra[P] == m and rb[P] == k, (letter, ra, rb)
        assert (np.diff(ra) >= 0).all() and (np.diff(rb) >= 0).all(), (letter, ra, rb)
    return out


def part_of(rp, ci, val, displs, r):
    """Rank r's slice as it passes it to init: the row pointer keeps its global offsets."""
    s, e = int(displs[r]), int(displs[r + 1])
    return rp[s:e + 1], ci[rp[s]:rp[e]], val[rp[s]:rp[e]]


class Data:
    """The exact and the rounded data of one matrix, generated on the GLOBAL pattern from a fixed seed and cached per width."""

    def __init__(self, name, rp, ci, m, k):
        self.name, self.rp, self.ci, self.m, self.k = name, rp, ci, m, k
        self.seed = sum(map(ord, name))
        self._cache = {}

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def exact64(self, n, wide):
        import fp64_ref
        rng = np.random.default_rng(self.seed + 1000 * n + (wide == "B"))
        return self._get(("x64", n, wide), lambda: fp64_ref.exact_parts(self.rp, self.ci, self.k, n, rng, wide))

    def exact64_second(self, n, wide):
        import fp64_ref
        rng = np.random.default_rng(self.seed + 1000 * n + 7)
        return self._get(("x64b", n, wide), lambda: fp64_ref.exact_parts(self.rp, self.ci, self.k, n, rng, wide, like=self.exact64(n, wide)))

    def exact32(self, n):
        import fp32_ref
        rng = np.random.default_rng(self.seed + 1000 * n + 3)
        return self._get(("x32", n), lambda: fp32_ref.exact_problem32(self.rp, self.ci, self.k, n, rng))

    def rounded64(self, n):
        import fp64_ref

        def make():
            val, B = fp64_ref.rounded_problem(self.rp, self.ci, self.k, n, np.random.default_rng(self.seed + 1000 * n + 5))
            return val, B, fp64_ref.f64_bound(self.rp, self.ci, val, B)
        return self._get(("r64", n), make)

    def rounded32(self, n):
        import fp32_ref

        def make():
            rng = np.random.default_rng(self.seed + 1000 * n + 6)
            val, B = fp32_ref.data_values(rng, int(self.rp[-1])), fp32_ref.data_B(rng, (self.k, n))
            return val, B, fp32_ref.f32_bound(self.rp, self.ci, val, B)
        return self._get(("r32", n), make)

    def exact_sets(self, n):
        """[(what, val64, B, C_exact)] -- fp64 with the wide integers in A, in B, and fp32."""
        a, b = self.exact64(n, "A"), self.exact64(n, "B")
        return [("f64 wide=A", a.val, a.B, a.C_exact), ("f64 wide=B", b.val, b.B, b.C_exact), ("f32",) + self.exact32(n)]

    def transposed(self):
        """(rowptr, colidx, order) of the transposed pattern, from a stable argsort of the column indices (np_transpose of
        tests/gpu_dist_t_worker.py): nonzero q of the transposed pattern is nonzero order[q] of A."""
        def make():
            order = np.argsort(self.ci, kind="stable")
            rows = np.repeat(np.arange(self.m, dtype=np.int32), np.diff(self.rp))
            rp_t = np.concatenate([[0], np.cumsum(np.bincount(self.ci, minlength=self.k))]).astype(np.int32)
            return rp_t, rows[order].astype(np.int32), order
        return self._get("t", make)

    def exact_t_sets(self, n):
        """[(what, val64 in A's order, B (m x n), C_exact (k x n))] for C = A^T B: the exact generators run on the TRANSPOSED pattern
        (their budgets follow its rows, A's columns), the values are carried back to A's order -- fp64 wide in A, in B, and fp32."""
        import fp32_ref
        import fp64_ref

        def make():
            rp_t, ci_t, order = self.transposed()

            def back(v_t):
                v = np.empty_like(v_t)
                v[order] = v_t
                return v
            out = []
            for i, wide in enumerate("AB"):
                x = fp64_ref.exact_parts(rp_t, ci_t, self.m, n, np.random.default_rng(self.seed + 1000 * n + 11 + i), wide)
                out.append(("exec_t f64 wide=" + wide, back(x.val), x.B, x.C_exact))
            v, B, C = fp32_ref.exact_problem32(rp_t, ci_t, self.m, n, np.random.default_rng(self.seed + 1000 * n + 13))
            return out + [("exec_t f32", back(v), B, C)]
        return self._get(("xt", n), make)

    def sddmm_set(self, n):
        """(val, X (m x n), Y (k x n), out0, out1) as float64, every number exact in fp32 too: X = 2^rx X0 and Y = 2^ry Y0 by rows,
        X0 and Y0 integers of magnitude 1 .. 255, exponents in [-8, 8], val = +-2^e with e in [-8, 8].  Every dot is an integer
        below n 255^2 < 2^22 times a power of two -- exact in fp32 and fp64 in any order, fused or not -- and so is its product
        with val: out0 (mode 0) and out1 (mode 1) are computed here in integers, never by the library."""
        def make():
            rng = np.random.default_rng(self.seed + 1000 * n + 17)
            nnz = int(self.rp[-1])
            ints = lambda shape: rng.integers(1, 256, size=shape) * (2 * rng.integers(0, 2, size=shape) - 1)
            X0, Y0 = ints((self.m, n)), ints((self.k, n))
            rx, ry = rng.integers(-8, 9, size=self.m), rng.integers(-8, 9, size=self.k)
            val = np.ldexp((2.0 * rng.integers(0, 2, size=nnz) - 1.0), rng.integers(-8, 9, size=nnz).astype(np.int32))
            rows, cols = np.repeat(np.arange(self.m), np.diff(self.rp)), self.ci[:nnz]
            assert np.abs(X0).max() <= 255 and np.abs(Y0).max() <= 255 and n * 255 * 255 < 2 ** 22, "exact SDDMM budget exceeded"
            D0 = np.einsum("pj,pj->p", X0[rows], Y0[cols])
            assert D0.dtype == np.int64 and (np.abs(D0) < 2 ** 22).all()
            X = np.ldexp(X0.astype(np.float64), rx.astype(np.int32)[:, None])
            Y = np.ldexp(Y0.astype(np.float64), ry.astype(np.int32)[:, None])
            out0 = np.ldexp(D0.astype(np.float64), (rx[rows] + ry[cols]).astype(np.int32))
            out1 = out0 * val
            tiny = float(np.finfo(np.float32).tiny)
            for a in (val, X, Y, out0, out1):
                assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and (np.abs(a[a != 0]) >= tiny).all(), "not exact in fp32"
            return val, X, Y, out0, out1
        return self._get(("sd", n), make)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


# ---------------------------------------------------------------------------------------------------------------- CPU half
def plan_only_main():
    import torch.distributed as dist
    import oracle as orc
    from crp_spmm_amd import comm as crp_comm, engine, gen, planner
    from dist_worker import emulate_exec

    crp_comm.init_process_group()
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    keys = ("A_rowptr", "A_colidx", "rB_nrow", "rB_self_nrow", "rB_self_src_ridxs", "rB_sridxs", "rB_rridxs", "rB_rcnts", "rB_scnts",
            "rB_rdispls", "rB_sdispls", "rB_recv_size")
    for name, rp, ci, m, k in matrices(gen):
        data = Data(name, rp, ci, m, k)
        for letter, ra, rb in partitions(planner, rp, m, k, P):
            s, e = int(ra[me]), int(ra[me + 1])
            for n in WIDTHS:
                x = data.exact64(n, "A")
                parts = [part_of(rp, ci, x.val, ra, r) for r in range(P)]
                eng = engine.RpSpmm(s, e - s, *parts[me], rb, n, world, plan_only=True)
                p = eng.plan()
                o = orc.rp_plan_all(parts, rb, n)[me]
                for key in keys:
                    assert np.array_equal(np.asarray(p[key]), np.asarray(o[key])), (me, name, letter, n, key)
                if p["rB_self_nrow"] > 0:
                    for key in ("rB_self_src_offset", "rB_self_dst_offset"):
                        assert p[key] == o[key], (me, name, letter, n, key)
                if name == "lower" and letter == "a":
                    assert me != 0 or (p["rB_recv_size"] == 0 and p["rB_sridxs"].size > 0), "rank 0 of `lower` sends and receives nothing"
                    assert me != P - 1 or p["rB_sridxs"].size == 0, "the last rank of `lower` sends nothing"
                C_loc = emulate_exec(p, world, np.ascontiguousarray(x.B[rb[me]:rb[me + 1]]), n, orc)
                assert C_loc.shape == (e - s, n) and np.array_equal(C_loc, x.C_exact[s:e]), (me, name, letter, n, "emulated product")
                eng.free()
            dist.barrier()
    if me == 0:
        print("DIST_LAYOUTS_PLAN_OK world=%d" % P)
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------- GPU half
class Operands:
    """B and C of one call: views inside larger buffers whose other elements hold SENT.  form: ("dev" | "host", layout, ld - n or
    ld - rows, offset of the view's first element in the buffer)."""

    def __init__(self, torch, dev, form, Bl, m, n):
        self.torch, self.where, self.layout = torch, form[0], form[1]
        pad, off = form[2], form[3]
        self.dt = Bl.dtype
        self.B_buf, self.B, self.B_dev = self._make(dev, Bl.shape[0], n, pad, off)
        self._view(self.B_buf, Bl.shape[0], n, pad, off)[...] = Bl if self.layout == 0 else Bl.T
        self.B_before = self.B_buf.copy()
        if self.where == "dev":
            self.B_dev.copy_(torch.from_numpy(self.B_buf))
        self.shape_c = (m, n, pad, off)
        self.C_buf, self.C, self.C_dev = self._make(dev, m, n, pad, off)

    def _ld(self, rows, n, pad):
        return ((rows, n), n + pad) if self.layout == 0 else ((n, rows + pad), rows + pad)

    def _view(self, flat, rows, n, pad, off):
        """The rows x n operand (layout 1: n x rows) inside the flat buffer."""
        shape, ld = self._ld(rows, n, pad)
        full = np.lib.stride_tricks.as_strided(flat[off:], shape=shape, strides=(ld * flat.itemsize, flat.itemsize), writeable=True)
        return full if self.layout == 0 else full[:, :rows]

    def _make(self, dev, rows, n, pad, off):
        """(the flat host image of the buffer, the operand to pass, the flat device buffer or None)."""
        torch = self.torch
        shape, ld = self._ld(rows, n, pad)
        flat = np.full(off + shape[0] * ld + 3, SENT, dtype=self.dt)
        if self.where == "host":
            return flat, np.lib.stride_tricks.as_strided(flat[off:], shape=shape, strides=(ld * flat.itemsize, flat.itemsize), writeable=True), None
        d = torch.full((flat.size,), SENT, dtype=torch.float64 if self.dt == np.float64 else torch.float32, device=dev)
        if rows == 0 and self.layout == 0 and pad == 0 and off == 0:
            # what a caller without rows has at hand: an empty tensor, whose pointer is NULL
            op = torch.empty((0, n), dtype=d.dtype, device=dev)
            assert op.data_ptr() == 0
            return flat, op, d
        return flat, d.as_strided(shape, (ld, 1), off), d

    def reset_c(self):
        """C := NaN inside, SENT around."""
        m, n, pad, off = self.shape_c
        self.C_buf[...] = SENT
        self._view(self.C_buf, m, n, pad, off)[...] = np.nan
        if self.where == "dev":
            self.C_dev.copy_(self.torch.from_numpy(self.C_buf))

    def result(self, tag):
        """The m x n product; asserts every sentinel of C intact and B's buffer unchanged."""
        m, n, pad, off = self.shape_c
        if self.where == "dev":
            self.torch.cuda.synchronize()
            got, b_now = self.C_dev.cpu().numpy(), self.B_dev.cpu().numpy()
        else:
            got, b_now = self.C_buf, self.B_buf
        assert np.array_equal(bits(b_now), bits(self.B_before)), tag + ("B was written",)
        inside = np.zeros(got.size, dtype=bool)
        self._view(inside, m, n, pad, off)[...] = True
        assert inside.sum() == m * n and (got[~inside] == SENT).all(), tag + ("an element outside C was written",)
        v = self._view(got, m, n, pad, off)
        return np.array(v if self.layout == 0 else v.T)


def forms(n):
    return [("dev", 0, 0, 0), ("dev", 0, 1, 1), ("dev", 0, 4, 0), ("dev", 1, 3, 0), ("host", 0, 3, 0), ("host", 1, 3, 0)]


def check_exact(torch, dev, call, set_timing, form, Bl, C_want, m, n, tag, reps=3):
    """One operand form: timing on, then off `reps` times; every result C_want bit for bit (a rank without rows: the call returns
    and nothing around C is touched)."""
    ops = Operands(torch, dev, form, Bl, m, n)
    first = None
    for timing, count in ((True, 1), (False, reps)):
        set_timing(timing)
        for rep in range(count):
            ops.reset_c()
            call(ops.layout, ops.B, ops.C)
            got = ops.result(tag + (form, timing, rep))
            assert got.shape == C_want.shape and got.dtype == C_want.dtype, tag
            if first is None:
                first = got
                same = np.array_equal(bits(got), bits(C_want)) if got.dtype == np.float32 else np.array_equal(got, C_want)
                if not same:
                    bad = np.argwhere(~(got == C_want))
                    raise AssertionError("%r %r: %d of %d entries differ from the exact product, first at %s: got %r, want %r"
                                         % (tag, form, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], C_want[tuple(bad[0])]))
            else:
                assert np.array_equal(bits(got), bits(first)), tag + (form, rep, "timing off differs from timing on")
    set_timing(True)


def check_sddmm(torch, dev, eng, form, Xl, Yl, wants, tag):
    """One operand form of the SDDMM, timing on and off, modes 0 and 1: `out` (on the device for device operands, on the host for
    host operands; empty on a rank without nonzeros) bit for bit wants[mode], the elements around it and X and Y untouched."""
    n, nnz = Xl.shape[1], wants[0].size
    ox, oy = Operands(torch, dev, form, Xl, 0, n), Operands(torch, dev, form, Yl, 0, n)
    for timing in (True, False):
        eng.set_timing(timing)
        for mode in (0, 1):
            t = tag + (form, timing, mode)
            if form[0] == "dev":
                buf = torch.full((nnz + 2,), SENT, dtype=ox.B_dev.dtype, device=dev)
                out = buf[1:1 + nnz] if nnz > 0 else torch.empty(0, dtype=buf.dtype, device=dev)
            else:
                buf = np.full(nnz + 2, SENT, dtype=Xl.dtype)
                out = buf[1:1 + nnz]
            eng.sddmm(ox.layout, ox.B, oy.B, out, mode)
            if form[0] == "dev":
                torch.cuda.synchronize()
                buf = buf.cpu().numpy()
                for o in (ox, oy):
                    assert np.array_equal(bits(o.B_dev.cpu().numpy()), bits(o.B_before)), t + ("an operand was written",)
            else:
                assert np.array_equal(bits(ox.B_buf), bits(ox.B_before)) and np.array_equal(bits(oy.B_buf), bits(oy.B_before)), t
            assert buf[0] == SENT and buf[-1] == SENT, t + ("an element outside out was written",)
            got, want = buf[1:1 + nnz], wants[mode]
            if not np.array_equal(bits(got), bits(want)):
                bad = np.flatnonzero(bits(got) != bits(want))
                raise AssertionError("%r: %d of %d entries differ from the exact SDDMM, first at %d: got %r, want %r"
                                     % (t, bad.size, nnz, bad[0], got[bad[0]], want[bad[0]]))
    eng.set_timing(True)


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
    mats = matrices(gen)
    datas = {name: Data(name, rp, ci, m, k) for name, rp, ci, m, k in mats}

    # ---- the row-parallel engine on every partition
    for name, rp, ci, m, k in mats:
        data = datas[name]
        for letter, ra, rb in partitions(planner, rp, m, k, P):
            s, e = int(ra[me]), int(ra[me + 1])
            bs, be = int(rb[me]), int(rb[me + 1])
            mine = slice(int(rp[s]), int(rp[e]))
            for n in WIDTHS:
                eng = None
                for what, val, B, C_exact in data.exact_sets(n):
                    tag = (me, name, letter, n, what)
                    if eng is None:
                        eng = engine.RpSpmm(s, e - s, rp[s:e + 1], ci[mine], val[mine], rb, n, world)
                        if letter == "a":
                            split = torch.tensor([int(min(eng.overlap_rows()) > 0)])
                            dist.all_reduce(split, op=dist.ReduceOp.MAX)
                            if name == "band":
                                assert int(split) == 1, (name, P, "no rank has the interior / boundary split")
                            if name == "lower":
                                p = eng.plan()
                                assert me != 0 or (p["rB_recv_size"] == 0 and p["rB_sridxs"].size > 0), tag
                                assert me != P - 1 or p["rB_sridxs"].size == 0, tag
                    else:
                        eng.update_values(val[mine])
                    Bl = np.ascontiguousarray(B[bs:be])
                    for form in forms(n):
                        check_exact(torch, dev, eng.exec, eng.set_timing, form, Bl, C_exact[s:e], e - s, n, tag)
                # ---- the transposed product and the SDDMM where a rank owns no row of A or of B: this rank's loc_B_nrow x n block of
                #      C = A^T B bit for bit (B has A's rows), `out` over this rank's nonzeros bit for bit; timing on once, off once
                if letter in T_LAYOUTS and n in T_WIDTHS:
                    for what, val, B, C_exact in data.exact_t_sets(n):
                        eng.update_values(val[mine])
                        call = eng.exec_t_f32 if B.dtype == np.float32 else eng.exec_t
                        for form in T_FORMS:
                            check_exact(torch, dev, call, eng.set_timing, form, np.ascontiguousarray(B[s:e]), C_exact[bs:be], be - bs, n,
                                        (me, name, letter, n, what), reps=1)
                    val, X, Y, out0, out1 = data.sddmm_set(n)
                    eng.update_values(val[mine])
                    # a rank without rows of B also passes what it has at hand for Y: an empty tensor, whose pointer is NULL (every rank
                    # runs that form when one has no rows: each call is an exchange all ranks take part in)
                    sd_forms = T_FORMS + ((("dev", 0, 0, 0),) if (np.diff(rb) == 0).any() else ())
                    for dt in (np.float64, np.float32):
                        for form in sd_forms:
                            check_sddmm(torch, dev, eng, form, np.ascontiguousarray(X[s:e], dtype=dt), np.ascontiguousarray(Y[bs:be], dtype=dt),
                                        (out0[mine].astype(dt), out1[mine].astype(dt)), (me, name, letter, n, "sddmm", np.dtype(dt).name))
                # ---- one multi-scale rounded case per matrix and partition: every entry of the rank's rows within the derived bound
                if n in (7, 24):
                    val, B, (ref, bound) = data.rounded64(n)
                    eng.update_values(val[mine])
                    ops = Operands(torch, dev, ("dev", 0, 1, 1), np.ascontiguousarray(B[bs:be]), e - s, n)
                    ops.reset_c()
                    eng.exec(0, ops.B, ops.C)
                    fp64_ref.check_f64_bound(rp[s:e + 1], None, None, None, ops.result((me, name, letter, n, "rounded f64")),
                                             what="rank %d %s (%s) n=%d rounded fp64" % (me, name, letter, n), ref_bound=(ref[s:e], bound[s:e]))
                    val, B, (ref, bound) = data.rounded32(n)
                    eng.update_values(val[mine])
                    ops = Operands(torch, dev, ("dev", 0, 1, 1), np.ascontiguousarray(B[bs:be]), e - s, n)
                    ops.reset_c()
                    eng.exec(0, ops.B, ops.C)
                    fp32_ref.check_f32_bound(rp[s:e + 1], None, None, None, ops.result((me, name, letter, n, "rounded f32")),
                                             what="rank %d %s (%s) n=%d rounded fp32" % (me, name, letter, n), ref_bound=(ref[s:e], bound[s:e]))
                # ---- every kernel variant and a second value set, on the nnz-balanced band at two ranks
                if name == "band" and letter == "a" and P == 2:
                    x = data.exact64(n, "A")
                    x2 = data.exact64_second(n, "A")
                    v32, B32, C32 = data.exact32(n)
                    for variant in (0, 1, 3, 5):
                        eng.set_variant(variant)
                        eng.update_values(x.val[mine])
                        check_exact(torch, dev, eng.exec, eng.set_timing, ("dev", 0, 0, 0), np.ascontiguousarray(x.B[bs:be]), x.C_exact[s:e],
                                    e - s, n, (me, name, n, "variant", variant), reps=1)
                        eng.update_values(x2.val[mine])
                        check_exact(torch, dev, eng.exec, eng.set_timing, ("dev", 0, 0, 0), np.ascontiguousarray(x2.B[bs:be]), x2.C_exact[s:e],
                                    e - s, n, (me, name, n, "variant", variant, "second value set"), reps=1)
                    eng.set_variant(0)
                    eng.update_values(v32[mine])
                    for variant in (0, 1, 5):
                        eng.set_variant_f32(variant)
                        check_exact(torch, dev, eng.exec, eng.set_timing, ("dev", 0, 0, 0), np.ascontiguousarray(B32[bs:be]), C32[s:e], e - s, n,
                                    (me, name, n, "f32 variant", variant), reps=1)
                eng.free()
            dist.barrier()

    # ---- the 2D engine on every pm x pn grid: AC_rowptr cuts A's rows into pm panels, B_rowptr cuts B's rows into pm blocks of its own,
    #      BC_colptr cuts the n columns evenly -- at n = 1 with pn > 1 some ranks hold no column
    grids = [(P // pn, pn, False) for pn in range(1, P + 1) if P % pn == 0] + [(P // 2, 2, True)]
    for name, rp, ci, m, k in mats:
        data = datas[name]
        for pm, pn, empty_slice in grids:
            if empty_slice and name != "band":
                continue
            pi, pj = me // pn, me % pn
            ac = np.asarray(planner.csr_mat_row_partition(rp, pm) if m == k else planner.even_displs(m, pm), dtype=np.int32)
            br = ac if m == k else np.asarray(planner.even_displs(k, pm), dtype=np.int32)
            a0 = np.zeros(P + 1, dtype=np.int32)
            for i in range(pm):
                a0[i * pn:(i + 1) * pn + 1] = planner.csr_mat_row_partition(rp[ac[i]:ac[i + 1] + 1] - rp[ac[i]], pn) + ac[i]
            if empty_slice:                              # the first rank of grid row 0 holds no rows of A0
                a0[0:2] = ac[0]
            assert a0[0] == 0 and a0[P] == m and (np.diff(a0) >= 0).all(), a0
            s0, e0 = int(a0[me]), int(a0[me + 1])
            r0, r1 = int(ac[pi]), int(ac[pi + 1])
            for n in WIDTHS:
                bc = planner.even_displs(n, pn)
                c0, c1 = int(bc[pj]), int(bc[pj + 1])
                e2 = None
                for what, val, B, C_exact in data.exact_sets(n):
                    tag = (me, name, "%dx%d%s" % (pm, pn, " empty slice" if empty_slice else ""), n, what)
                    if e2 is None:
                        e2 = engine.Para2dSpmm(world, pm, pn, a0, br, ac, bc, rp[s0:e0 + 1], ci[rp[s0]:rp[e0]], val[rp[s0]:rp[e0]])
                    else:
                        e2.update_values(val[rp[s0]:rp[e0]])
                    Bl = np.ascontiguousarray(B[br[pi]:br[pi + 1], c0:c1])
                    Cw = np.ascontiguousarray(C_exact[r0:r1, c0:c1])
                    for form in (("dev", 0, 1, 1), ("host", 1, 3, 0)):
                        check_exact(torch, dev, e2.exec, e2.rp.set_timing, form, Bl, Cw, r1 - r0, c1 - c0, tag, reps=1)
                e2.free()
            dist.barrier()
    if me == 0:
        print("GPU_DIST_LAYOUTS_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    if "--plan-only" in sys.argv[1:]:
        plan_only_main()
    else:
        gpu_main()
