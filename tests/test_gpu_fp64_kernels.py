"""GPU (MI355X): the fp64 SpMM kernels instance by instance, on exact data and by the entrywise fp64 error bound (tests/fp64_ref.py).

Every product of this module
* runs on exact_problem data (both `wide` settings: the 27-bit side in A's values, then in B) into a C prefilled with NaN,
* must give C_exact entry for entry (torch.equal / np.array_equal: a NaN left behind differs, -0.0 == +0.0),
* must leave C's padding columns and the rows outside a row map untouched,
* records the kernel instance it launched (crp_csr_dev_last_kernel) in SEEN; the failure message carries the instance, the matrix, the
  width and the first wrong (row, column).
The last test, the census, asserts that all 67 fp64 instances have run: row-group 12, column-major 1, row-panel 32, narrow 6, team2r 4,
team2 12.  It reads what the tests before it recorded, so it needs the whole module to have run (no -k selection).

The exact data cannot exercise rounding: test_rounded_data_within_bound runs one width per instance class on data of many scales against
check_f64_bound and prints the worst ratio.

Matrices: random_csr(777, 1234, 70 | 150) with every 13th row empty, kkt3d(10) (mostly-hole panels: compact values), fem3d(8) / fem3d(12)
(the locality order needs 2048 rows), the 9000-row stride lattice (team schedule of the row-panel kernels), a dense band of 1100 rows
(filled panels: the narrow kernel's full values), the 13- and 64-row matrices of the row-owner kernel's test."""
import numpy as np
import pytest

import fp64_ref as F

pytestmark = pytest.mark.gpu

WIDES = ("A", "B")
SEEN = {}            # kernel instance -> the first case that launched it; filled by _product, read by the census (the last test)
NMAX = 1026          # every exact problem is generated once at this width; narrower operands are its first columns

ROWGROUP = ["rowgroup<%d,%d,%d>" % t for t in ((4, 2, 1), (8, 2, 1), (16, 2, 1), (32, 2, 1), (64, 2, 1), (64, 2, 2),
                                                (4, 1, 1), (8, 1, 1), (16, 1, 1), (32, 1, 1), (64, 1, 1), (64, 1, 2))]
PANEL = ["panel<%d,%d,%d,%s,%s>" % (R, NV, VW, a, b) for R in (4, 8) for NV, VW in ((1, 1), (2, 1), (1, 2), (2, 2))
         for a in ("a32", "a64") for b in ("b0", "b1")]
NARROW = ["narrow<b0,o32,compact>", "narrow<b0,o32,full>", "narrow<b0,o64,compact>", "narrow<b0,o64,full>",
          "narrow<b1,o64,compact>", "narrow<b1,o64,full>"]
TEAM2R = ["team2r<%d,%s>" % (G, b) for G in (4, 2) for b in ("b0", "b1")]
TEAM2 = ["team2<f64,%s,%s,%s>" % (nv, b, c) for nv in ("NVH", "NV1", "NV2") for b in ("b0", "b1") for c in ("compact", "full")]
INSTANCES = ROWGROUP + ["cm"] + PANEL + NARROW + TEAM2R + TEAM2
assert len(INSTANCES) == len(set(INSTANCES)) == 67

_MATS, _PROBS = {}, {}


def _matrix(name):
    """(rowptr, colidx, number of columns)."""
    if name not in _MATS:
        from crp_spmm_amd import gen
        nx, ny, nz = 300, 6, 5
        make = {"random70": lambda: gen.random_csr(777, 1234, 70, seed=11, empty_every=13),
                "random150": lambda: gen.random_csr(777, 1234, 150, seed=12, empty_every=13),
                "kkt3d": lambda: gen.kkt3d(10), "fem3d8": lambda: gen.fem3d(8), "fem3d12": lambda: gen.fem3d(12),
                "lattice": lambda: gen.banded_fem(nx * ny * nz, offsets=(1, 2, 3, 4, 5, nx, nx + 1, nx * ny, nx * ny + 1), seed=4),
                "band": lambda: gen.banded_fem(1100, offsets=(1, 2, 3, 4, 5, 6, 7, 8), seed=3),
                "tiny13": lambda: gen.random_csr(13, 40, 5, seed=1), "tiny64": lambda: gen.random_csr(64, 40, 36, seed=7),
                "past4g": _past4g_matrix}[name]
        rp, ci, _ = make()
        k = {"random70": 1234, "random150": 1234, "tiny13": 40, "tiny64": 40, "past4g": 1100}.get(name, rp.size - 1)
        _MATS[name] = (np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32), k)
    return _MATS[name]


def _past4g_matrix():
    """1500 x 1100, up to 40 per row, the last rows of B named by every fifth nonzero (test_b_block_beyond_4gib's)."""
    from crp_spmm_amd import gen
    rp, ci, va = gen.random_csr(1500, 1100, 40, seed=21)
    ci = ci.copy()
    ci[::5] = 1100 - 1 - (ci[::5] % 7)
    for r in range(1500):
        ci[rp[r]:rp[r + 1]] = np.sort(ci[rp[r]:rp[r + 1]])
    return rp, ci, va


class _Problem:
    """An exact problem on the host and (lazily) on the device."""

    def __init__(self, name, wide, rp, ci, k, parts):
        self.name, self.wide, self.rp, self.ci, self.k, self.m = name, wide, rp, ci, k, rp.size - 1
        self.parts, self.val, self.B, self.Cx = parts, parts.val, parts.B, parts.C_exact
        self._dev = None

    def dev(self, gpu):
        """(B, C_exact) on the device."""
        import torch
        if self._dev is None:
            self._dev = (torch.from_numpy(self.B).to(gpu), torch.from_numpy(self.Cx).to(gpu))
        return self._dev

    def second(self, seed):
        """The same pattern, exponents and B with new integers in A: for value updates."""
        parts = F.exact_parts(self.rp, self.ci, self.k, self.B.shape[1], np.random.default_rng(seed), self.wide, like=self.parts)
        Q = _Problem(self.name + " (value set %d)" % seed, self.wide, self.rp, self.ci, self.k, parts)
        if self._dev is not None:
            import torch
            Q._dev = (self._dev[0], torch.from_numpy(Q.Cx).to(self._dev[0].device))
        return Q


def _problem(name, wide, nmax=NMAX, pattern=None):
    """The exact problem of a matrix (or of `pattern` = (rowptr, colidx, k) under that name), cached."""
    key = (name, wide, nmax)
    if key not in _PROBS:
        rp, ci, k = pattern or _matrix(name)
        rng = np.random.default_rng([len(name), ord(name[0]), ord(name[-1]), int(wide == "B"), nmax])
        _PROBS[key] = _Problem(name, wide, rp, ci, k, F.exact_parts(rp, ci, k, nmax, rng, wide))
    return _PROBS[key]


def _operand(Xd, n, ldpad=0, off=0, rows=None):
    """The first n columns of the device matrix Xd (of its rows `rows`: a slice or an index array) as a view of ld = n + ldpad + off
    columns starting `off` elements into its row (off = 1: not 16-byte aligned); the rest of the allocation is zero."""
    import torch
    if rows is not None:
        Xd = Xd[rows if isinstance(rows, slice) else torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(Xd.device)]
    big = torch.zeros((Xd.shape[0], n + ldpad + off), dtype=torch.float64, device=Xd.device)
    big[:, off:off + n] = Xd[:, :n]
    return big[:, off:off + n]


def _explain(got, want, what):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    bad = np.argwhere(~(g == w))
    i, j = (int(x) for x in bad[0])
    return ("%s: %d entries in %d rows differ from C_exact; first at (row %d, col %d): C = %r, exact = %r; rows %s ..."
            % (what, bad.shape[0], np.unique(bad[:, 0]).size, i, j, g[i, j], w[i, j], np.unique(bad[:, 0])[:8].tolist()))


def _product(A, B0, B1, n, variant, Cxd, what, family, ldpad=0, offc=0, mapped=False):
    """One row-major product into a fresh NaN-filled C (ld = n + ldpad + offc, starting offc elements into the row; with `mapped` the handle
    carries the row map i -> 2 i + 1 into 2 m + 1 rows): C == C_exact, nothing else written, the instance is of `family` and recorded."""
    import torch
    from crp_spmm_amd import hip
    m = A.nrow
    big = torch.full((2 * m + 1 if mapped else m, n + ldpad + offc), float("nan"), dtype=torch.float64, device=Cxd.device)
    Cv = big[:, offc:offc + n]
    hip.spmm_csr(A, B0, Cv, n=n, B1=B1, variant=variant)
    torch.cuda.synchronize()
    name = A.last_kernel
    what = "%s n=%d variant %d [%s]" % (what, n, variant, name)
    assert name.startswith(family), (what, "expected an instance of", family)
    SEEN.setdefault(name, what)
    got = Cv[1::2] if mapped else Cv
    want = Cxd[:, :n]
    if not torch.equal(got, want):
        raise AssertionError(_explain(got, want, what))
    assert bool(torch.isnan(big[:, :offc]).all()) and bool(torch.isnan(big[:, offc + n:]).all()), (what, "C padding columns written")
    if mapped:
        assert bool(torch.isnan(Cv[0::2]).all()), (what, "a row outside the row map was written")
    return name


class _Handles:
    """The handles of one problem: one source (B0 = B), two sources (B0 = rows [k/3, 2k/3) of B, B1 = the rest) and B0 = NULL."""

    def __init__(self, P, gpu):
        self.P, self.gpu, self.made = P, gpu, {}
        self.lo, self.hi = P.k // 3, (2 * P.k) // 3
        self.codes, self.remote = F.split_two_source(P.ci, P.k, self.lo, self.hi)

    def get(self, src):
        from crp_spmm_amd import hip
        if src not in self.made:
            P = self.P
            if src == "b0":
                self.made[src] = hip.CsrDev(P.m, P.k, P.rp, P.ci, P.val)
            elif src == "b1":
                self.made[src] = hip.CsrDev(P.m, self.hi - self.lo, P.rp, self.codes, P.val)
            else:
                self.made[src] = hip.CsrDev(P.m, 1, P.rp, (~P.ci).astype(np.int32), P.val)
        return self.made[src]

    def run(self, src, n, variant, family, ldpad=0, offb=0, offc=0, mapped=False, extra=""):
        """src: "b0", "b1" (two sources) or "null" (B0 = NULL, every code negative).  ldpad / offb apply to every B operand."""
        Bd, Cxd = self.P.dev(self.gpu)
        A = self.get(src)
        if src == "b0":
            B0, B1 = _operand(Bd, n, ldpad, offb), None
        elif src == "b1":
            B0, B1 = _operand(Bd, n, ldpad, offb, slice(self.lo, self.hi)), _operand(Bd, n, ldpad, offb, self.remote)
        else:
            B0, B1 = None, _operand(Bd, n, ldpad, offb)
        what = "%s wide=%s %s ldpad=%d offb=%d offc=%d%s%s" % (self.P.name, self.P.wide, src, ldpad, offb, offc, " row map" if mapped else "", extra)
        return _product(A, B0, B1, n, variant, Cxd, what, family, ldpad, offc, mapped)

    def free(self):
        for A in self.made.values():
            A.free()
        self.made = {}


def _vw(name):
    return int(name.split("<")[1].rstrip(">").split(",")[1])


@pytest.mark.parametrize("wide", WIDES)
def test_rowgroup_exact(crp, gpu, wide):
    """Variant 1 (csrc/spmm_kernels.hip, spmm_rm_f64_kernel): the vector path at aligned even n on both sides of every bucket, the scalar
    path at odd n, at even n with ld = n + 1 and at even n with B or C one element off 16-byte alignment; two sources, B0 = NULL, a row
    map into 2 m + 1 rows; every matrix at two widths."""
    H = _Handles(_problem("random150", wide, 520), gpu)
    for n in (2, 8, 10, 16, 18, 32, 34, 64, 66, 128, 130, 258, 520):
        assert _vw(H.run("b0", n, 1, "rowgroup<")) == 2, (n, "an aligned even operand left the vector path")
    for n in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 129, 257):
        assert _vw(H.run("b0", n, 1, "rowgroup<", ldpad=1 - n % 2)) == 1, n
    for n in (4, 8, 34, 130):                      # an even ld and a pointer 8 bytes off: B alone, C alone
        assert _vw(H.run("b0", n, 1, "rowgroup<", ldpad=1, offb=1)) == 1, n
        assert _vw(H.run("b0", n, 1, "rowgroup<", ldpad=1, offc=1)) == 1, n
    for n in (2, 10, 33, 130):
        H.run("b1", n, 1, "rowgroup<")
        H.run("null", n, 1, "rowgroup<")
    A = H.get("b0")
    A.set_rowmap(np.arange(H.P.m, dtype=np.int32) * 2 + 1, 2 * H.P.m + 1)
    for n in (2, 10, 33, 130):
        H.run("b0", n, 1, "rowgroup<", mapped=True)
    H.free()
    for name in ("random70", "kkt3d", "fem3d8", "lattice", "tiny13"):
        H = _Handles(_problem(name, wide), gpu)
        for n in (18, 65):
            H.run("b0", n, 1, "rowgroup<")
            H.run("b1", n, 1, "rowgroup<")
        H.free()


@pytest.mark.parametrize("wide", WIDES)
def test_column_major_exact(crp, gpu, wide):
    """layout = 1 (spmm_cm_f64_kernel): operands as (n, ld) tensors with padded leading dimensions, plain and through a row map."""
    import torch
    from crp_spmm_amd import hip
    for name in ("random70", "kkt3d", "fem3d8", "lattice"):
        P = _problem(name, wide)
        Bd, Cxd = P.dev(gpu)
        A = hip.CsrDev(P.m, P.k, P.rp, P.ci, P.val)
        for mapped in (False, True):
            if mapped:
                A.set_rowmap(np.arange(P.m, dtype=np.int32) * 2 + 1, 2 * P.m + 1)
            crows = 2 * P.m + 1 if mapped else P.m
            for n in (1, 5, 33):
                Bt = torch.zeros((n, P.k + 3), dtype=torch.float64, device=gpu)
                Bt[:, :P.k] = Bd[:, :n].T
                Ct = torch.full((n, crows + 2), float("nan"), dtype=torch.float64, device=gpu)
                hip.spmm_csr(A, Bt, Ct, n=n, layout=1)
                torch.cuda.synchronize()
                what = "%s wide=%s column-major n=%d%s [%s]" % (name, wide, n, " row map" if mapped else "", A.last_kernel)
                assert A.last_kernel == "cm", what
                SEEN.setdefault("cm", what)
                got = (Ct[:, 1:crows:2] if mapped else Ct[:, :crows]).T
                if not torch.equal(got, Cxd[:, :n]):
                    raise AssertionError(_explain(got, Cxd[:, :n], what))
                assert bool(torch.isnan(Ct[:, crows:]).all()), (what, "C padding written")
                if mapped:
                    assert bool(torch.isnan(Ct[:, 0:crows:2]).all()), (what, "a row outside the row map was written")
        A.free()


@pytest.mark.parametrize("wide", WIDES)
@pytest.mark.parametrize("R", [4, 8])
def test_panel_exact(crp, gpu, R, wide):
    """Variants 2 and 3 (spmm_panel_f64_kernel<R, NV, VW, ADDR64, HAS_B1>), the four (NV, VW) shapes with one and two sources: (1, 1) at
    n <= 64, (2, 1) at n > 64 odd or with ld = n + 1, (1, 2) at even 64 < n <= 128, (2, 2) above; the lattice matrix from 128 columns on,
    where the waves of a workgroup follow the team schedule (psync).  (R = 8 at even 24 <= n <= 32 is the narrow kernel's.)"""
    variant, fam = (2, "panel<4,") if R == 4 else (3, "panel<8,")
    w11 = (25, 33, 34, 64) + ((24, 32) if R == 4 else (31,))
    cases = [(n, 0) for n in w11 + (65, 129, 66, 100, 128, 130, 256, 258, 520)] + [(130, 1), (66, 1)]
    shapes = set()
    H = _Handles(_problem("random70", wide), gpu)
    for n, ldpad in cases:
        for src in ("b0", "b1"):
            shapes.add(tuple(H.run(src, n, variant, fam, ldpad=ldpad).split(",")[1:3]))
    H.get("b0").set_rowmap(np.arange(H.P.m, dtype=np.int32) * 2 + 1, 2 * H.P.m + 1)
    for n in (33, 129, 100, 258):
        H.run("b0", n, variant, fam, mapped=True)
    H.free()
    assert shapes == {("1", "1"), ("2", "1"), ("1", "2"), ("2", "2")}, shapes
    for name, some in (("kkt3d", ((33, 0), (65, 0), (100, 0), (258, 0))), ("fem3d8", ((33, 0), (65, 0), (100, 0), (258, 0))),
                       ("lattice", ((64, 0), (128, 0), (129, 0), (130, 1), (256, 0), (520, 0)))):
        H = _Handles(_problem(name, wide), gpu)
        for n, ldpad in some:
            for src in ("b0", "b1"):
                H.run(src, n, variant, fam, ldpad=ldpad)
        H.free()


@pytest.mark.parametrize("wide", WIDES)
def test_narrow_exact(crp, gpu, wide):
    """The narrow-operand kernel (csrc/narrow_kernel.hip; variant 3 at even 24 <= n <= 32, aligned): compact values (random, kkt3d: under
    60 % of the panels' (row, entry) pairs exist) and full values (the dense band), one source (32-bit offsets) and two, leading-dimension
    pads 0 / 2 / 6, a row map."""
    kinds = {}
    for name in ("random70", "kkt3d", "band", "lattice"):
        H = _Handles(_problem(name, wide), gpu)
        for n in (24, 26, 30, 32):
            for ldpad in (0, 2, 6):
                for src in ("b0", "b1"):
                    kinds[name] = H.run(src, n, 3, "narrow<", ldpad=ldpad).rstrip(">").split(",")[2]
        H.get("b0").set_rowmap(np.arange(H.P.m, dtype=np.int32) * 2 + 1, 2 * H.P.m + 1)
        H.run("b0", 30, 3, "narrow<", mapped=True)
        H.free()
    assert kinds["kkt3d"] == "compact" and kinds["band"] == "full", kinds


@pytest.mark.parametrize("wide", WIDES)
def test_team2r_exact(crp, gpu, wide):
    """Variant 7, the row-owner team kernel (csrc/team2r_kernel.hip): G = 4 at n = 24, 30, 32 and G = 2 at n = 34, 48, 64, one and two
    sources, padded leading dimensions; random / KKT / lattice matrices and the 13- and 64-row ones (a single, ragged team)."""
    for name in ("random70", "kkt3d", "lattice", "tiny13", "tiny64"):
        H = _Handles(_problem(name, wide), gpu)
        for n in (24, 30, 32, 34, 48, 64):
            for src in ("b0", "b1"):
                got = H.run(src, n, 7, "team2r<")
                assert got == "team2r<%d,%s>" % (4 if n <= 32 else 2, src), (name, n, got)
            H.run("b0", n, 7, "team2r<", ldpad=2)
        H.get("b0").set_rowmap(np.arange(H.P.m, dtype=np.int32) * 2 + 1, 2 * H.P.m + 1)
        for n in (30, 48):
            H.run("b0", n, 7, "team2r<", mapped=True)
        H.free()


TEAM2_WIDTHS = (24, 26, 62, 64, 66, 126, 128, 130, 254, 256, 258, 510, 512, 514, 1026)


@pytest.mark.parametrize("wide", WIDES)
@pytest.mark.parametrize("compact", [1, 0])
def test_team2_exact(crp, gpu, monkeypatch, compact, wide):
    """Variant 5, the LDS-sharing team kernel (csrc/team2_kernel.hip and its 12 hand-written round loops in team2_consume.inc): the half
    piece (n <= 64), one piece (<= 128) and two pieces (256-column tiles: partial pieces, partial tiles, several tiles), one and two
    sources, compact and full value blocks (CRPSPMM_TEAM2_COMPACT before the first product of a fresh handle)."""
    lib = crp.load()
    monkeypatch.setenv("CRPSPMM_TEAM2_COMPACT", str(compact))
    fam = "team2<f64,"
    for name, widths in (("random70", TEAM2_WIDTHS), ("fem3d8", TEAM2_WIDTHS), ("kkt3d", (24, 64, 66, 128, 130, 514)),
                         ("lattice", (26, 62, 126, 258, 1026))):
        H = _Handles(_problem(name, wide), gpu)
        for n in widths:
            for src in ("b0", "b1"):
                got = H.run(src, n, 5, fam, extra=" compact=%d" % compact)
                assert got.endswith(",compact>" if compact else ",full>"), (name, n, got)
                assert lib.crp_csr_dev_team2_compact(H.get(src).handle) == compact, (name, n)
        H.run("b0", 130, 5, fam, ldpad=2)
        H.get("b0").set_rowmap(np.arange(H.P.m, dtype=np.int32) * 2 + 1, 2 * H.P.m + 1)
        for n in (62, 126, 258):
            H.run("b0", n, 5, fam, mapped=True)
        H.free()


def test_b_rows_past_4gib_exact(crp, gpu):
    """B rows addressed past 4 GiB (one allocation of 1100 rows with ld = 2^19 doubles; only the first columns of each row hold data, the
    last rows are named): the row-panel kernels' 64-bit addresses in all four shapes for R = 4 and R = 8, with B0 alone and with B0 + a
    small B1; the narrow kernel's 64-bit offsets on compact and on full values; the team kernel at 128 and 258 columns."""
    import torch
    from crp_spmm_amd import hip
    k, ld, nmax = 1100, 1 << 19, 258
    Bbig = torch.empty((k, ld), dtype=torch.float64, device=gpu)
    assert Bbig.numel() * 8 > (1 << 32) and (k - 8) * ld * 8 > (1 << 32)
    handles = []
    try:
        for wide in WIDES:
            for name, jobs in (("past4g", [(2, n, "panel<4,") for n in (33, 129, 100, 258)] + [(3, n, "panel<8,") for n in (33, 129, 100, 258)] +
                                [(3, 32, "narrow<"), (5, 128, "team2<f64,"), (5, 258, "team2<f64,")]),
                               ("band", [(3, 32, "narrow<"), (3, 258, "panel<8,")])):
                P = _problem(name, wide, nmax)
                assert P.k == k and int(P.ci.max()) == k - 1
                Bd, Cxd = P.dev(gpu)
                Bbig[:, :nmax] = Bd
                # two sources: B0 = rows 0 .. 1089 of the big allocation (still past 4 GiB), B1 = the last ten rows, small
                codes, remote = F.split_two_source(P.ci, k, 0, k - 10)
                assert (k - 10) * ld * 8 > (1 << 32) and int(codes.max()) >= (1 << 32) // (ld * 8) and (codes < 0).any()
                A0 = hip.CsrDev(P.m, k, P.rp, P.ci, P.val)
                A1 = hip.CsrDev(P.m, k - 10, P.rp, codes, P.val)
                handles += [A0, A1]
                for variant, n, fam in jobs:
                    what = "%s wide=%s past 4 GiB" % (name, wide)
                    got = _product(A0, Bbig[:, :n], None, n, variant, Cxd, what + " b0", fam)
                    assert fam == "team2<f64," or "64" in got, (what, n, got, "the 32-bit addressing instance ran")
                    got = _product(A1, Bbig[:k - 10, :n], _operand(Bd, n, 0, 0, remote), n, variant, Cxd, what + " b1", fam)
                    assert fam == "team2<f64," or "64" in got, (what, n, got)
                for A in (A0, A1):
                    A.free()
    finally:
        for A in handles:
            A.free()
        del Bbig
        torch.cuda.empty_cache()


FAMILIES = {"rowgroup": (1, 33, "rowgroup<"), "panel4": (2, 100, "panel<4,"), "panel8": (3, 130, "panel<8,"), "narrow": (3, 32, "narrow<"),
            "team2": (5, 128, "team2<f64,"), "team2r": (7, 32, "team2r<")}


@pytest.mark.parametrize("wide", WIDES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_value_updates_exact(crp, gpu, monkeypatch, family, wide):
    """crp_csr_dev_update_values with a host pointer, then a device pointer, on a handle whose format exists (built before the update)
    and on fresh handles (the format is built after it): every product equals C_exact of the value set it was given last -- a slot
    map that sends one value to the wrong slot cannot hide in a small row."""
    import torch
    from crp_spmm_amd import hip
    monkeypatch.delenv("CRPSPMM_TEAM2_COMPACT", raising=False)
    variant, n, fam = FAMILIES[family]
    P1 = _problem("fem3d8", wide)
    Bd, _ = P1.dev(gpu)
    P2, P3 = P1.second(2), P1.second(3)
    assert not np.array_equal(P1.Cx[:, :n], P2.Cx[:, :n]) and not np.array_equal(P2.Cx[:, :n], P3.Cx[:, :n])
    B0 = _operand(Bd, n)
    v3d = torch.from_numpy(P3.val).to(gpu)
    what = "fem3d8 wide=%s update " % wide
    A = hip.CsrDev(P1.m, P1.k, P1.rp, P1.ci, P1.val)
    _product(A, B0, None, n, variant, P1.dev(gpu)[1], what + "before", fam)
    A.update_values(P2.val)
    _product(A, B0, None, n, variant, P2.dev(gpu)[1], what + "host pointer, format built before", fam)
    A.update_values(v3d)
    _product(A, B0, None, n, variant, P3.dev(gpu)[1], what + "device pointer, format built before", fam)
    A.free()
    A = hip.CsrDev(P1.m, P1.k, P1.rp, P1.ci, P1.val)
    A.update_values(P2.val)
    _product(A, B0, None, n, variant, P2.dev(gpu)[1], what + "host pointer, format built after", fam)
    A.free()
    A = hip.CsrDev(P1.m, P1.k, P1.rp, P1.ci, P1.val)
    A.update_values(v3d)
    _product(A, B0, None, n, variant, P3.dev(gpu)[1], what + "device pointer, format built after", fam)
    A.free()


def _transposed_pattern(rp, ci, k):
    """(rowptr, colidx) of A^T and perm: entry q of A^T (row-major) is entry perm[q] of A."""
    m = rp.size - 1
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    perm = np.argsort(ci, kind="stable")
    rpT = np.zeros(k + 1, dtype=np.int32)
    rpT[1:] = np.cumsum(np.bincount(ci, minlength=k))
    return rpT, rows[perm], perm


@pytest.mark.parametrize("wide", WIDES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_from_transpose_exact(crp, gpu, monkeypatch, family, wide):
    """CsrDev.from_transpose (the device transpose) of the rectangular random matrix, whose transpose has empty rows: the product equals
    C_exact of the numpy-transposed problem; then new values in A's order."""
    from crp_spmm_amd import hip
    monkeypatch.delenv("CRPSPMM_TEAM2_COMPACT", raising=False)
    variant, n, fam = FAMILIES[family]
    rp, ci, k = _matrix("random70")
    m = rp.size - 1
    rpT, ciT, perm = _transposed_pattern(rp, ci, k)
    PT = _problem("random70^T", wide, 130, pattern=(rpT, ciT, m))
    Bd, Cxd = PT.dev(gpu)

    def in_a_order(vT):
        v = np.empty_like(vT)
        v[perm] = vT
        return v
    At = hip.CsrDev.from_transpose(m, k, rp, ci, in_a_order(PT.val))
    assert At.is_transposed and At.nrow == k
    what = "random70^T wide=%s from_transpose" % wide
    _product(At, _operand(Bd, n), None, n, variant, Cxd, what, fam)
    P2 = PT.second(4)
    At.update_values(in_a_order(P2.val))
    _product(At, _operand(Bd, n), None, n, variant, P2.dev(gpu)[1], what + " after update_values", fam)
    At.free()


@pytest.mark.parametrize("wide", WIDES)
def test_locality_order_exact(crp, gpu, monkeypatch, wide):
    """Formats in the locality order (CRPSPMM_REORDER=1, fem3d(12)), every family at one width, plain and with a caller row map on top:
    every row lands where the caller expects it."""
    from crp_spmm_amd import hip
    lib = crp.load()
    monkeypatch.setenv("CRPSPMM_REORDER", "1")
    monkeypatch.delenv("CRPSPMM_TEAM2_COMPACT", raising=False)
    P = _problem("fem3d12", wide, 130)
    Bd, Cxd = P.dev(gpu)
    A = hip.CsrDev(P.m, P.k, P.rp, P.ci, P.val)
    assert lib.crp_csr_dev_reordered(A.handle) == 1
    for mapped in (False, True):
        if mapped:
            A.set_rowmap(np.arange(P.m, dtype=np.int32) * 2 + 1, 2 * P.m + 1)
        for family in sorted(FAMILIES):
            variant, n, fam = FAMILIES[family]
            _product(A, _operand(Bd, n), None, n, variant, Cxd, "fem3d12 wide=%s locality order%s" % (wide, " row map" if mapped else ""),
                     fam, mapped=mapped)
    A.free()


# one width per instance class: (matrix, variant, n, ldpad, two sources, CRPSPMM_TEAM2_COMPACT or None)
ROUNDED = {
    "rowgroup": [("random150", 1, n, 0, False, None) for n in (8, 16, 32, 64, 128, 130, 3, 5, 9, 17, 33, 65)] + [("random150", 1, 130, 0, True, None)],
    "panel": [(name, v, n, 0, two, None) for name in ("random70", "lattice") for v in (2, 3) for n, two in ((33, False), (129, False), (100, False), (258, False), (100, True))],
    "narrow": [(name, 3, 32, 0, two, None) for name in ("kkt3d", "band") for two in (False, True)],
    "team2r": [(name, 7, n, 0, two, None) for name in ("kkt3d", "random70") for n, two in ((32, False), (64, False), (32, True))],
    "team2": [(name, 5, n, 0, two, cp) for name in ("fem3d8", "kkt3d") for cp in (1, 0) for n, two in ((64, False), (128, False), (258, False), (128, True))],
}


@pytest.mark.parametrize("family", sorted(ROUNDED) + ["cm"])
def test_rounded_data_within_bound(crp, gpu, monkeypatch, family):
    """Ordinary rounded data on many scales (rows of A over 24 decades, rows of B over 12) through one width of every instance class:
    |C - ref| <= 1.0001 (L_i + 1) 2^-53 (|A| |B|) entrywise against np.longdouble (check_f64_bound), no entry left out; prints the worst
    ratio of every case."""
    import torch
    from crp_spmm_amd import hip
    cache = {}
    cases = ROUNDED.get(family) or [(name, 1, 5, 0, False, None) for name in ("random70", "kkt3d")]
    for name, variant, n, ldpad, two, compact in cases:
        rp, ci, k = _matrix(name)
        m = rp.size - 1
        if (name, n) not in cache:
            val, B = F.rounded_problem(rp, ci, k, n, np.random.default_rng([k, n]))
            cache[(name, n)] = (val, B, F.f64_bound(rp, ci, val, B), torch.from_numpy(B).to(gpu))
        val, B, rb, Bd = cache[(name, n)]
        if compact is None:
            monkeypatch.delenv("CRPSPMM_TEAM2_COMPACT", raising=False)
        else:
            monkeypatch.setenv("CRPSPMM_TEAM2_COMPACT", str(compact))
        lo, hi = k // 3, (2 * k) // 3
        codes, remote = F.split_two_source(ci, k, lo, hi)
        A = hip.CsrDev(m, hi - lo if two else k, rp, codes if two else ci, val)
        if family == "cm":
            Bt = torch.zeros((n, k + 3), dtype=torch.float64, device=gpu)
            Bt[:, :k] = Bd.T
            Ct = torch.full((n, m + 2), float("nan"), dtype=torch.float64, device=gpu)
            hip.spmm_csr(A, Bt, Ct, n=n, layout=1)
            torch.cuda.synchronize()
            got = Ct[:, :m].T.cpu().numpy().copy()
        else:
            big = torch.full((m, n + ldpad), float("nan"), dtype=torch.float64, device=gpu)
            B0, B1 = (_operand(Bd, n, ldpad, 0, slice(lo, hi)), _operand(Bd, n, ldpad, 0, remote)) if two else (_operand(Bd, n, ldpad), None)
            hip.spmm_csr(A, B0, big[:, :n], n=n, B1=B1, variant=variant)
            torch.cuda.synchronize()
            got = big[:, :n].cpu().numpy().copy()
        kernel = A.last_kernel
        A.free()
        what = "%s rounded data n=%d variant %d%s [%s]" % (name, n, variant, " two sources" if two else "", kernel)
        worst = F.check_f64_bound(rp, ci, val, B, got, what, ref_bound=rb)
        print("%-70s worst |C - ref| / bound = %.3f" % (what, worst))
        SEEN.setdefault(kernel, what)


def test_census_every_fp64_instance_ran():
    """Every one of the 67 fp64 kernel instances was launched (and therefore checked exactly) by the tests above, and nothing ran
    under a name this list does not know."""
    f64 = {k: v for k, v in SEEN.items() if "f32" not in k}
    missing = [k for k in INSTANCES if k not in f64]
    unknown = sorted(set(f64) - set(INSTANCES))
    print("fp64 kernel instances launched: %d of %d" % (len(INSTANCES) - len(missing), len(INSTANCES)))
    assert not unknown, ("instances the census does not list", unknown)
    assert not missing, ("fp64 kernel instances never launched (%d of %d ran)" % (len(INSTANCES) - len(missing), len(INSTANCES)), missing)
