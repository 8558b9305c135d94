"""GPU (MI355X): the fp32 SpMM kernels instance by instance, by exact references and by the fp32 error bound (tests/fp32_ref.py).

* CSR row-group kernel (csrc/spmm_f32.hip, variant 1): bit for bit against csr_f32_sequential -- every <LPR, VW> instance on both
  sides of its width bucket, padded and misaligned operands (scalar path), two sources, B0 = NULL, caller row maps.
* Team kernel (csrc/team2_kernel.hip, variant 5): each of its 12 fp32 instances (NV x one / two sources x compact / full value
  blocks) within check_f32_bound; exact invariants of its structure (fp32 and fp64): column slices, compact = full, padded leading
  dimensions, repeats.
* Non-finite B, value updates in both build orders, the locality order with a caller row map, B rows past 4 GiB.

Which case launches each instance:
  row-group <LPR, VW>  vec4 (n % 4 == 0, ld pad 0 or 4, aligned): <4,4> n = 4, 8, 12, 16; <8,4> 20, 32; <16,4> 36, 64; <32,4> 100, 128;
                       <64,4> 132, 256, 260, 516, 1024.  Scalar (every n with ld pad 1 or a misaligned operand; n % 4 != 0 always):
                       <4,1> n = 1 .. 4; <8,1> 5, 8; <16,1> 12, 16; <32,1> 17, 20, 32; <64,1> 33 and up -- test_rowgroup_f32_bit_exact
  team2 fp32           NVH (n <= 128): 24, 28, 124, 128; NV1 (129 .. 256): 132, 252, 256; NV2 (> 256): 260 .. 1028; each with B0 alone and
                       B0 + B1, compact and full value blocks -- the 12 instances, all in test_team2_f32_every_instance_within_bound

Data rule (fp32_ref): values and B entries are +-2^U(-8, 1).  Every product checks the variant it launched
(crp_csr_dev_last_variant) and that C's padding columns and sentinel rows are untouched."""
import ctypes as C

import numpy as np
import pytest

import fp32_ref as F

pytestmark = pytest.mark.gpu

_IP = C.POINTER(C.c_int)

# the row-group kernel: LPR buckets 4 / 8 / 16 / 32 / 64 of the vec4 path (n <= 16, 32, 64, 128, more) and of the scalar path
# (n <= 4, 8, 16, 32, more), both sides of each bucket
ROWGROUP_WIDTHS = [1, 2, 3, 4, 5, 8, 12, 16, 17, 20, 32, 33, 36, 64, 65, 100, 128, 129, 132, 256, 260, 300, 516, 1024]
# the team kernel: NV = 0 (n <= 128), 1 (129 .. 256), 2 (> 256: 512-column tiles); partial pieces, partial tiles, several tiles
TEAM_WIDTHS = [24, 28, 124, 128, 132, 252, 256, 260, 388, 508, 512, 516, 1024, 1028]


def _nv(n):
    return 2 if n > 256 else (1 if n > 128 else 0)


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _operand(X, dev, ldpad=0, off=0, dtype=None):
    """X on the device as a view of ld = n + ldpad + off columns starting `off` elements into its row (off = 1: not 16-byte aligned);
    the rest of the allocation is zero."""
    import torch
    dt = dtype or (torch.float32 if X.dtype == np.float32 else torch.float64)
    n = X.shape[1]
    big = torch.zeros((X.shape[0], n + ldpad + off), dtype=dt, device=dev)
    big[:, off:off + n] = _t(X, dev)
    return big[:, off:off + n]


def _product(lib, A, B0, n, variant, want, B1=None, c_rows=None, ldpad=0, off=0, fill=float("nan"), f64=False):
    """One product into a fresh C of c_rows rows (ld = n + ldpad + off, starting `off` elements into the row) filled with `fill`; checks
    the launched variant and that nothing outside the C view changed.  Returns the whole C (numpy) and its view's columns."""
    import torch
    from crp_spmm_amd import hip
    c_rows = A.nrow if c_rows is None else c_rows
    big = torch.full((c_rows, n + ldpad + off), fill, dtype=torch.float64 if f64 else torch.float32, device=B1.device if B0 is None else B0.device)
    Cv = big[:, off:off + n]
    if f64:
        hip.spmm_csr(A, B0, Cv, n=n, B1=B1, variant=variant)
    else:
        hip.spmm_csr_f32(A, B0, Cv, n=n, B1=B1, variant=variant)
    torch.cuda.synchronize()
    got = lib.crp_csr_dev_last_variant(A.handle)
    assert got == want, ("launched variant", got, "wanted", want, n)
    out = big.cpu().numpy()
    outside = np.concatenate([out[:, :off], out[:, off + n:]], axis=1)
    assert (np.isnan(outside) if np.isnan(fill) else (outside == fill)).all(), ("C padding columns written", n)
    return out, out[:, off:off + n]


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                 b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


_split_two_source = F.split_two_source


def _rowgroup_matrix(n):
    """777 rows (not a multiple of any rows-per-block), empty rows, rows of up to 150 entries (several 64-pair chunks)."""
    from crp_spmm_amd import gen
    rp, ci, _ = gen.random_csr(777, 1234, 150, seed=100 + n, empty_every=13)
    rng = np.random.default_rng(n)
    return rp, ci, F.data_values(rng, ci.size), F.data_B(rng, (1234, n))


@pytest.mark.parametrize("n", ROWGROUP_WIDTHS)
def test_rowgroup_f32_bit_exact(crp, gpu, n):
    """Variant 1 = csr_f32_sequential bit for bit: leading-dimension pads 0 / 1 / 4, B or C one float off 16-byte alignment (the scalar
    path), the two-source column index, B0 = NULL with every code negative, and a caller row map into a taller C."""
    from crp_spmm_amd import hip
    lib = crp.load()
    rp, ci, va, B = _rowgroup_matrix(n)
    m, k = rp.size - 1, B.shape[0]
    ref = F.csr_f32_sequential(rp, ci, va, B)
    assert not ref[::13].any()
    A = hip.CsrDev(m, k, rp, ci, va)
    for ldpad, offb, offc in ((0, 0, 0), (1, 0, 0), (4, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        Bd = _operand(B, gpu, ldpad, offb)
        _, got = _product(lib, A, Bd, n, 1, 1, ldpad=ldpad, off=offc)
        assert _bits_equal(got, ref), (n, ldpad, offb, offc)
    A.free()
    # two sources (B0 = local rows, B1 = receive buffer), and B0 = NULL with every column in B1: the same sums, the same bits
    codes, remote = _split_two_source(ci, k, 300, 650)
    A = hip.CsrDev(m, 350, rp, codes, va)
    _, got = _product(lib, A, _operand(B[300:650], gpu), n, 1, 1, B1=_operand(B[remote], gpu, 1 if n % 4 else 0))
    assert _bits_equal(got, ref), (n, "two sources")
    A.free()
    A = hip.CsrDev(m, 1, rp, (~ci).astype(np.int32), va)
    _, got = _product(lib, A, None, n, 1, 1, B1=_operand(B, gpu))
    assert _bits_equal(got, ref), (n, "B0 = NULL")
    A.free()
    # caller row map into 2m + 1 rows: odd rows hold the product, even rows keep their fill
    A = hip.CsrDev(m, k, rp, ci, va)
    rowmap = (np.arange(m, dtype=np.int32) * 2 + 1)
    assert lib.crp_csr_dev_set_rowmap(A.handle, rowmap.ctypes.data_as(_IP), 2 * m + 1) == 0
    _, got = _product(lib, A, _operand(B, gpu), n, 1, 1, c_rows=2 * m + 1, fill=7.0)
    assert _bits_equal(got[1::2], ref), (n, "row map")
    assert (got[0::2] == 7.0).all(), (n, "row map: a sentinel row was written")
    A.free()


def _team_matrices():
    from crp_spmm_amd import gen
    nx, ny, nz = 300, 6, 5
    out = [("random", gen.random_csr(777, 1234, 70, seed=11, empty_every=13), 1234),            # ragged last team, empty rows
           ("lattice", gen.banded_fem(nx * ny * nz, offsets=(1, 2, 3, 4, 5, nx, nx + 1, nx * ny, nx * ny + 1), seed=4), nx * ny * nz),
           ("kkt3d", gen.kkt3d(10), None),                                                     # mostly-hole panels
           ("fem3d", gen.fem3d(12), None)]                                                     # the Queen-class stand-in
    res = []
    for i, (name, (rp, ci, _), k) in enumerate(out):
        k = k or rp.size - 1
        res.append((name, rp, ci, F.data_values(np.random.default_rng(50 + i), ci.size), k))
    return res


def test_team2_f32_every_instance_within_bound(crp, gpu, monkeypatch):
    """Variant 5 in fp32 on four matrices (random with empty rows and a ragged last team, a stride lattice, a KKT system, the fem3d
    stand-in) at every width class, one and two B sources, compact and full value blocks (CRPSPMM_TEAM2_COMPACT before the first
    product of a fresh handle): every product within check_f32_bound; at the end every one of the 12 fp32 instances
    (NV, B1, COMPACT) has run."""
    from crp_spmm_amd import hip
    lib = crp.load()
    seen = {}
    for name, rp, ci, va, k in _team_matrices():
        m = rp.size - 1
        rng = np.random.default_rng(m)
        Bs = {n: F.data_B(rng, (k, n)) for n in TEAM_WIDTHS}
        bounds = {n: F.f32_bound(rp, ci, va, Bs[n]) for n in TEAM_WIDTHS}
        lo, hi = k // 3, (2 * k) // 3
        codes, remote = _split_two_source(ci, k, lo, hi)
        for compact in (1, 0):
            monkeypatch.setenv("CRPSPMM_TEAM2_COMPACT", str(compact))
            for two in (False, True):
                A = hip.CsrDev(m, hi - lo if two else k, rp, codes if two else ci, va)
                for n in TEAM_WIDTHS:
                    B = Bs[n]
                    if two:
                        B0, B1 = _operand(B[lo:hi], gpu), _operand(B[remote], gpu, 4)
                    else:
                        B0, B1 = _operand(B, gpu), None
                    _, got = _product(lib, A, B0, n, 5, 5, B1=B1, ldpad=4)
                    assert lib.crp_csr_dev_team2_compact(A.handle) == compact, (name, n)
                    what = "%s n=%d %s %s" % (name, n, "compact" if compact else "full", "B0+B1" if two else "B0")
                    F.check_f32_bound(rp, ci, va, B, got, what, ref_bound=bounds[n])
                    seen.setdefault((_nv(n), two, bool(compact)), what)
                A.free()
    missing = [(nv, b1, cp) for nv in (0, 1, 2) for b1 in (False, True) for cp in (False, True) if (nv, b1, cp) not in seen]
    assert not missing, ("fp32 team instances never launched", missing)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_team2_exact_invariants(crp, gpu, monkeypatch, dtype):
    """What the team kernel's structure makes exact, on the fem3d stand-in and the random matrix (fp32 and fp64 variant 5): each
    (row, column) of C is the same FMA sequence in the format's round order whatever tile or instance covers it, so (i) C at width w is
    bit-identical to the first w columns of C at width 1028 (one handle); (ii) compact and full value blocks give the same C (two
    handles; array_equal, as a hole of a full block may add an exact zero: -0 == +0); (iii) padded leading dimensions and (iv) a
    repeated product are bit-identical."""
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    f64 = dtype == "f64"
    npdt = np.float64 if f64 else np.float32
    widths = (24, 128, 256, 512)
    cases = [("fem3d", gen.fem3d(12)), ("random", gen.random_csr(777, 777, 70, seed=12, empty_every=13))]
    for name, (rp, ci, _) in cases:
        m = rp.size - 1
        rng = np.random.default_rng(7)
        va = F.data_values(rng, ci.size)
        Bw = F.data_values(rng, (m, 1028)).astype(npdt)
        full = {}
        for compact in (1, 0):
            monkeypatch.setenv("CRPSPMM_TEAM2_COMPACT", str(compact))
            A = hip.CsrDev(m, m, rp, ci, va)
            _, c1028 = _product(lib, A, _operand(Bw, gpu), 1028, 5, 5, f64=f64)
            assert lib.crp_csr_dev_team2_compact(A.handle) == compact
            if not f64:
                F.check_f32_bound(rp, ci, va, Bw, c1028, "%s fp32 1028" % name)
            full[compact] = {1028: c1028}
            for w in widths:
                Bv = np.ascontiguousarray(Bw[:, :w])
                _, cw = _product(lib, A, _operand(Bv, gpu), w, 5, 5, f64=f64)
                assert _bits_equal(cw, np.ascontiguousarray(c1028[:, :w])), ("(i) column slice", name, dtype, compact, w)
                _, cp = _product(lib, A, _operand(Bv, gpu, 4), w, 5, 5, ldpad=4, f64=f64)
                assert _bits_equal(cp, cw), ("(iii) padded leading dimensions", name, dtype, compact, w)
                _, cr = _product(lib, A, _operand(Bv, gpu), w, 5, 5, f64=f64)
                assert _bits_equal(cr, cw), ("(iv) repeat", name, dtype, compact, w)
                full[compact][w] = cw
            A.free()
        for w in (1028,) + widths:
            assert np.array_equal(full[1][w], full[0][w]), ("(ii) compact = full", name, dtype, w)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("compact", [1, 0])
def test_team2_f32_nonfinite(crp, gpu, monkeypatch, compact):
    """Inf and NaN rows of B next to absent pairs on each NV (fp32 variant 5) and through the row-group kernel: C's NaN and Inf
    positions equal the fp64 oracle's, the finite entries are within the bound -- an absent pair is never multiplied (no 0 * Inf)."""
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    monkeypatch.setenv("CRPSPMM_TEAM2_COMPACT", str(compact))
    m, k = 500, 900
    rp, ci, _ = gen.random_csr(m, k, 30, seed=2)
    rng = np.random.default_rng(3)
    va = F.data_values(rng, ci.size)
    A = hip.CsrDev(m, k, rp, ci, va)
    for n in (124, 252, 516):
        B = F.data_B(rng, (k, n))
        used = np.unique(ci)
        B[used[::17]] = np.inf
        B[used[3::23], ::3] = -np.inf
        B[used[5::29]] = np.nan
        for variant in (5, 1):
            _, got = _product(lib, A, _operand(B, gpu), n, variant, variant, ldpad=4)
            F.check_f32_bound(rp, ci, va, B, got, "nonfinite n=%d variant %d compact %d" % (n, variant, compact))
            assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got).any()
    assert lib.crp_csr_dev_team2_compact(A.handle) == compact
    A.free()


@pytest.mark.parametrize("order", ["f64_first", "f32_first"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_team2_f32_value_updates(crp, gpu, monkeypatch, order, where):
    """crp_csr_dev_update_values with a host or device pointer once the team format exists: built by an fp64 product (compact value
    blocks; the fp32 values are derived at the first fp32 product, after the update) or by an fp32 product (full blocks, fp32 values
    derived before the update).  Each fp32 product after the update is within the bound of the NEW values and differs from the old one;
    the row-group kernel's stays bit-exact."""
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    monkeypatch.delenv("CRPSPMM_TEAM2_COMPACT", raising=False)
    rp, ci, _ = gen.fem3d(8)
    m = rp.size - 1
    rng = np.random.default_rng(4)
    va = F.data_values(rng, ci.size)
    v2 = F.data_values(rng, ci.size)
    widths = (128, 256, 516)
    Bs = {n: F.data_B(rng, (m, n)) for n in widths}
    A = hip.CsrDev(m, m, rp, ci, va)
    old = {}
    if order == "f64_first":
        _product(lib, A, _operand(Bs[128].astype(np.float64), gpu), 128, 5, 5, f64=True)
        assert lib.crp_csr_dev_team2_compact(A.handle) == 1           # fp64 builds compact blocks; no fp32 product before the update
    else:
        for n in widths:
            _, old[n] = _product(lib, A, _operand(Bs[n], gpu), n, 5, 5)
            F.check_f32_bound(rp, ci, va, Bs[n], old[n], "before the update n=%d" % n)
            _product(lib, A, _operand(Bs[n], gpu), n, 1, 1)
        assert lib.crp_csr_dev_team2_compact(A.handle) == 0           # an fp32 product first keeps full blocks (fill >= 0.4)
    vals = np.ascontiguousarray(v2) if where == "host" else _t(v2, gpu)
    assert lib.crp_csr_dev_update_values(A.handle, vals.ctypes.data if where == "host" else vals.data_ptr(), None) == 0
    for n in widths:
        B = Bs[n]
        _, got5 = _product(lib, A, _operand(B, gpu), n, 5, 5)
        F.check_f32_bound(rp, ci, v2, B, got5, "after the update n=%d %s %s" % (n, order, where))
        ref_old, _ = F.f32_bound(rp, ci, va, B)
        assert not np.allclose(got5, ref_old, rtol=1e-3), (n, order, where, "still the old values")
        if n in old:
            assert not np.array_equal(got5, old[n]), (n, order, where, "still the old result")
        _, got1 = _product(lib, A, _operand(B, gpu), n, 1, 1)
        assert _bits_equal(got1, F.csr_f32_sequential(rp, ci, v2, B)), (n, order, where)
    A.free()
    torch.cuda.synchronize()


def test_locality_order_f32(crp, gpu, monkeypatch):
    """Formats in the locality order (CRPSPMM_REORDER=1 on a shell mesh): fp32 variants 0, 1 and 5 at n = 64, 132, 516 put every row
    where the caller expects it -- variant 1 bit-exact (CSR in the caller's order), variant 5 within the bound, variant 0 the host plan's
    choice -- and with a caller row map into 2m + 1 rows: odd rows the product, even rows untouched."""
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    rp, ci, _ = gen.shell_fem(nc=24, nl=40, m=24 * 40 * 6 - 3, seam_to=30)
    m = rp.size - 1
    rng = np.random.default_rng(8)
    va = F.data_values(rng, ci.size)
    monkeypatch.setenv("CRPSPMM_REORDER", "1")
    widths = (64, 132, 516)
    _, plan = hip.spmm_plan_host(rp, ci, widths, variant=0, dtype="f32")
    A = hip.CsrDev(m, m, rp, ci, va)
    assert lib.crp_csr_dev_reordered(A.handle) == 1
    Bs = {n: F.data_B(rng, (m, n)) for n in widths}
    seq = {n: F.csr_f32_sequential(rp, ci, va, Bs[n]) for n in widths}
    for mapped in (False, True):
        if mapped:
            rowmap = (np.arange(m, dtype=np.int32) * 2 + 1)
            assert lib.crp_csr_dev_set_rowmap(A.handle, rowmap.ctypes.data_as(_IP), 2 * m + 1) == 0
        for n, v0 in zip(widths, plan):
            for variant, want in ((0, v0), (1, 1), (5, 5)):
                _, got = _product(lib, A, _operand(Bs[n], gpu), n, variant, want, c_rows=2 * m + 1 if mapped else m, fill=7.0)
                if mapped:
                    assert (got[0::2] == 7.0).all(), (n, variant, "row map: a sentinel row was written")
                    got = got[1::2]
                what = "locality n=%d variant %d%s" % (n, variant, " row map" if mapped else "")
                if want == 1:
                    assert _bits_equal(got, seq[n]), what
                else:
                    F.check_f32_bound(rp, ci, va, Bs[n], got, what)
    A.free()


def test_f32_b_rows_past_4gib(crp, gpu):
    """B rows addressed past 4 GiB in fp32 (ld = 2^20 floats, 1100 rows: 4.6 GB, only n columns of each row hold data): variant 1
    bit-exact, variant 5 (its 64-bit row addresses) within the bound."""
    import torch
    from crp_spmm_amd import gen, hip
    lib = crp.load()
    k, ld, m = 1100, 1 << 20, 1500
    rp, ci, _ = gen.random_csr(m, k, 40, seed=21)
    ci = ci.copy()
    ci[::5] = k - 1 - (ci[::5] % 7)                      # the last rows (beyond 4 GiB) are hit
    for r in range(m):
        ci[rp[r]:rp[r + 1]] = np.sort(ci[rp[r]:rp[r + 1]])
    rng = np.random.default_rng(22)
    va = F.data_values(rng, ci.size)
    nmax = 260
    B = F.data_B(rng, (k, nmax))
    Bbig = torch.empty((k, ld), dtype=torch.float32, device=gpu)
    assert Bbig.numel() * 4 > (1 << 32) and (k - 8) * ld * 4 > (1 << 32)
    Bbig[:, :nmax] = _t(B, gpu)
    A = hip.CsrDev(m, k, rp, ci, va)
    try:
        for n in (128, 260):
            Bv = Bbig[:, :n]
            _, got1 = _product(lib, A, Bv, n, 1, 1)
            assert _bits_equal(got1, F.csr_f32_sequential(rp, ci, va, B[:, :n])), n
            _, got5 = _product(lib, A, Bv, n, 5, 5)
            F.check_f32_bound(rp, ci, va, B[:, :n], got5, "past 4 GiB n=%d" % n)
    finally:
        A.free()
        del Bbig
        torch.cuda.empty_cache()
