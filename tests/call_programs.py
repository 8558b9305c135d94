"""Seeded programs of calls on one handle pair and on one engine, with the model that predicts them (no GPU: numpy, the matrix
generators and the built library's host-side planning calls crp_spmm_plan_host / crp_panel_format_host; helper module
of tests/test_call_programs_data.py and tests/test_gpu_call_programs.py; not a conftest).

A PROGRAM is a list of steps, plain tuples that print as replayable literals: ``(kind, stream, parameters ...)``.  It owns one
matrix, a list of value sets drawn in advance on that matrix's pattern, and (device handle programs) a ``CsrDev`` of A and a
``CsrDev.from_transpose`` of the same A, which every update keeps on the same values.

The MODEL holds what a correct library must hold -- the current value vector in A's order, the current row map and c_nrow, and
which pieces of lazily built state exist and what built them -- and predicts from these alone every output and every query.

VALUE SETS share one pattern, one set of exponents and one set of operands, so that an update changes nothing but the values:

    val[p] = a0[p] 2^(re[i] + ce[c])         B = 2^-ce[c] B0[c, :]   (A B)         Bt = 2^-re[i] Bt0[i, :]   (A^T Bt)
    X = 2^rx[i] X0[i, :],  Y = 2^ry[c] Y0[c, :]                              (SDDMM)

    E32   a0 odd below 2^BA: with |B0|, |Bt0| odd below 2^BB and L = the longest row or column, L 2^BA 2^BB <= 2^24: every product,
          transposed product and partial sum is an integer below 2^24 times a power of two -- ONE correct bit pattern in fp32 and
          therefore in fp64.  |X0|, |Y0| <= 15 and at most 64 columns: a dot is below 2^14, times a0 below 2^24.
    E64   a0 odd below 2^27 (fp64_ref's "wide" construction): exact in fp64 only (27 + BB + 4 <= 52; a dot times a0 below 2^41);
          an fp32 call rounds the value once, so it is checked by the fp32 bounds.  This is what catches a value that went
          through a float.
    R     uniform(-2, 2): checked by the derived bounds.

The exponent ranges are narrower than fp32_ref's (re in [-8, 8], ce in [-4, 4] against [-20, 20] and [-10, 10]): the values are
the bias of the attention steps, and the narrower range keeps more than one probability of a row above fp32's underflow; under
an E set the bias is still steep, which is why those steps are compared with a fresh handle and not with the derived bounds.

The model's products are formed here in int64, never by the library and never by the oracle.
"""
import functools
from collections import namedtuple

import numpy as np

import fp32_ref

RE, CE, RXY = 8, 4, 4
NMAX = 130                      # widest product operand
SD_NMAX = 64                    # widest SDDMM / attention operand
SD_MAG = 15
WIDE_BITS = 27
WIDTHS = (1, 7, 24, 26, 32, 40, 64, 130)
PADS = (0, 1, 2, 6)
SD_WIDTHS = (1, 7, 24, 40, 64)
ATTN_WIDTHS = ((8, 40), (24, 24), (7, 26))
VARIANTS64 = (0, 1, 2, 3, 5, 7)
VARIANTS32 = (0, 1, 5)
PIECES = ("pan4", "pan8", "team2", "tval32", "t2r4", "t2r2", "val32")
SITUATIONS = ("fresh", "host", "dev")
OUT_EXTRA = 13                  # positions of an out_pos target that no nonzero names


# ---- the matrices ---------------------------------------------------------------------------------------------------------------

Pattern = namedtuple("Pattern", "name m k rp gcol rows codes ncol0 lo hi remote rpt cit tmap")


def _sparse_panels(block=128, per_row=8):
    """384 x 256: row i of block b = i / 128 names the columns base(b) + ((i mod 128) + 8 j) mod 128, j < 8, with base 0 for the
    blocks 0 and 2 and 128 for block 1.  No two rows of an R = 8 panel share a column (its panels are 7/8 holes), while 64
    consecutive rows name 120 columns with 512 nonzeros (the team formats pay).  Blocks 0 and 2 share their columns and block 1
    shares none with them, so the breadth-first order of the panel groups (16 panels: one block at R = 8) is 0, 2, 1: not the
    identity."""
    i = np.arange(3 * block)
    base = np.where(i // block == 1, block, 0)
    cols = np.sort(base[:, None] + ((i % block)[:, None] + 8 * np.arange(per_row)[None, :]) % block, axis=1)
    return (np.arange(3 * block + 1) * per_row).astype(np.int32), cols.reshape(-1).astype(np.int32)


def _base(name):
    from crp_spmm_amd import gen
    if name == "band":
        rp, ci, _ = gen.banded_fem(384, offsets=tuple(range(1, 8)))           # filled panels: 15 of 22 (row, entry) pairs
        return rp, ci, 384, 384
    if name == "band2048":      # the smallest square matrix whose handle may hold its rows in another order (format_order: 2048 rows)
        rp, ci, _ = gen.banded_fem(2048, offsets=tuple(range(1, 8)))
        return rp, ci, 2048, 2048
    if name == "rect":
        rp, ci, _ = gen.random_csr(300, 260, 12, empty_every=7)
        return rp, ci, 300, 260
    if name == "sparse":
        rp, ci = _sparse_panels()
        return rp, ci, 384, 256
    raise KeyError(name)


MATRICES = ("band", "rect", "sparse")


@functools.lru_cache(maxsize=None)
def pattern(name, two_source):
    """The pattern in the HANDLE's order.  two_source: columns [k / 4, k / 4 + k / 2) are B0's rows, the rest B1's (codes ~c),
    re-sorted inside the rows as tests/test_gpu_fuzz.py does -- so a row's entries are not in ascending column order."""
    rp, ci, m, k = _base(name)
    rp = rp.astype(np.int32)
    rows = np.repeat(np.arange(m), np.diff(rp))
    if two_source:
        lo, hi = k // 4, k // 4 + k // 2
        codes, remote = fp32_ref.split_two_source(ci.astype(np.int64), k, lo, hi)
        key = np.where(codes < 0, ~codes.astype(np.int64), codes.astype(np.int64) + (1 << 31))
        order = np.lexsort((key, rows))
        codes, gcol, ncol0 = codes[order].astype(np.int32), ci[order].astype(np.int32), hi - lo
    else:
        lo, hi, remote, codes, gcol, ncol0 = 0, k, np.zeros(0, np.int64), ci.astype(np.int32), ci.astype(np.int32), k
    tmap = np.lexsort((rows, gcol)).astype(np.int32)            # A^T in the stable transposed order
    rpt = np.concatenate([[0], np.cumsum(np.bincount(gcol, minlength=k))]).astype(np.int32)
    for a in (rp, gcol, rows, codes, remote, rpt, tmap):
        a.setflags(write=False)
    cit = rows[tmap].astype(np.int32)
    cit.setflags(write=False)
    return Pattern(name, m, k, rp, gcol, rows, codes, ncol0, lo, hi, remote, rpt, cit, tmap)


def seg_sum(t, rp):
    """per row of rp, the sum of the rows of t (one per nonzero), in t's dtype"""
    out = np.zeros((rp.size - 1,) + t.shape[1:], t.dtype)
    ne = np.flatnonzero(np.diff(rp) > 0)
    if ne.size:
        out[ne] = np.add.reduceat(t, rp[ne].astype(np.intp), axis=0)
    return out


# ---- the value sets -------------------------------------------------------------------------------------------------------------

ValueSet = namedtuple("ValueSet", "kind a0 val")


class Data:
    """The exponents, the operands and the value sets of one program (see the module's docstring)."""

    def __init__(self, pat, seed, kinds):
        rng = np.random.default_rng(seed)
        self.pat = pat
        m, k, nnz = pat.m, pat.k, pat.gcol.size
        self.longest = max(int(np.diff(pat.rp).max()), int(np.diff(pat.rpt).max()), 1)
        room = 24 - int(np.ceil(np.log2(self.longest)))
        self.ba, self.bb = room // 2, room - room // 2
        assert self.longest <= 16 and self.ba >= 10 and self.bb >= 10, ("the fp32 budget must leave 10 bits a side", self.longest)
        odd = lambda bits, size: (2 * rng.integers(0, 1 << (bits - 1), size=size, dtype=np.int64) + 1) * (2 * rng.integers(0, 2, size=size) - 1)
        small = lambda shape: rng.integers(1, SD_MAG + 1, size=shape) * (2 * rng.integers(0, 2, size=shape) - 1)
        self.re, self.ce = rng.integers(-RE, RE + 1, size=m), rng.integers(-CE, CE + 1, size=k)
        self.rx, self.ry = rng.integers(-RXY, RXY + 1, size=m), rng.integers(-RXY, RXY + 1, size=k)
        self.B0, self.Bt0 = odd(self.bb, (k, NMAX)), odd(self.bb, (m, NMAX))
        self.X0, self.Y0 = small((m, SD_NMAX)), small((k, SD_NMAX))
        self.B = np.ldexp(self.B0.astype(np.float64), (-self.ce).astype(np.int32)[:, None])
        self.Bt = np.ldexp(self.Bt0.astype(np.float64), (-self.re).astype(np.int32)[:, None])
        self.X = np.ldexp(self.X0.astype(np.float64), self.rx.astype(np.int32)[:, None])
        self.Y = np.ldexp(self.Y0.astype(np.float64), self.ry.astype(np.int32)[:, None])
        self.vexp = (self.re[pat.rows] + self.ce[pat.gcol]).astype(np.int32)
        self.sets = []
        for kind in kinds:
            if kind == "R":
                self.sets.append(ValueSet("R", None, rng.uniform(-2.0, 2.0, size=nnz)))
            else:
                a0 = odd(self.ba if kind == "E32" else WIDE_BITS, nnz)
                self.sets.append(ValueSet(kind, a0, np.ldexp(a0.astype(np.float64), self.vexp)))
        # attention operands: standard normal, scale 1 / sqrt(nk) (attention_ref.operands); the upstream gradient with them
        self.Q = rng.standard_normal((m, SD_NMAX))
        self.K = rng.standard_normal((k, SD_NMAX))
        self.V = rng.standard_normal((k, SD_NMAX))
        self.dO = rng.standard_normal((m, SD_NMAX))
        self.scores = rng.uniform(-4.0, 4.0, size=nnz)          # row softmax: a spread of 8, inside softmax_ref's data rule
        self.grads = rng.standard_normal(nnz)
        self.out_pos = rng.permutation(nnz + OUT_EXTRA)[:nnz].astype(np.int32)
        self.rowmaps = {1: (rng.permutation(m + 37)[:m].astype(np.int32), m + 37), 2: (rng.permutation(m + 5)[:m].astype(np.int32), m + 5)}
        for a in (self.B, self.Bt, self.X, self.Y, self.Q, self.K, self.V, self.dO, self.scores, self.grads, self.out_pos):
            a.setflags(write=False)

    # -- the exact budgets: sum |a0| |b0| over every row, every column and every dot
    def budgets(self, vs):
        """{name: (largest sum, limit)} for an E set"""
        pat = self.pat
        lim = 2 ** 24 if vs.kind == "E32" else 2 ** 53
        a = np.abs(vs.a0)
        rows = seg_sum(a[:, None] * np.abs(self.B0)[pat.gcol], pat.rp).max()
        cols = seg_sum(a[pat.tmap][:, None] * np.abs(self.Bt0)[pat.cit], pat.rpt).max()
        dots = (np.abs(self.X0)[pat.rows] * np.abs(self.Y0)[pat.gcol]).sum(axis=1)
        return {"rows": (int(rows), lim), "columns": (int(cols), lim), "dots": (int(dots.max()), lim),
                "dots times value": (int((dots * a).max()), lim)}

    # -- the model's exact results (E sets), as float64 arrays that are exact in the dtype they are compared in
    def product(self, vs, n):
        c0 = seg_sum(vs.a0[:, None] * self.B0[self.pat.gcol, :n], self.pat.rp)
        return np.ldexp(c0.astype(np.float64), self.re.astype(np.int32)[:, None])

    def product_t(self, vs, n):
        pat = self.pat
        c0 = seg_sum(vs.a0[pat.tmap][:, None] * self.Bt0[pat.cit, :n], pat.rpt)
        return np.ldexp(c0.astype(np.float64), self.ce.astype(np.int32)[:, None])

    def sddmm(self, vs, mode, n):
        """exact for mode 0 under every set, for mode 1 under an E set"""
        pat = self.pat
        d0 = (self.X0[pat.rows, :n] * self.Y0[pat.gcol, :n]).sum(axis=1)
        e = (self.rx[pat.rows] + self.ry[pat.gcol]).astype(np.int32)
        if mode == 0:
            return np.ldexp(d0.astype(np.float64), e)
        return np.ldexp((d0 * vs.a0).astype(np.float64), e + self.vexp)


def exact_in(kind, dtype):
    """whether a result that depends on the values has one correct bit pattern in this dtype under this kind of set"""
    return kind == "E32" or (kind == "E64" and dtype == "f64")


# ---- the kernel choice, restated (csrc/dispatch.cpp); tests/test_call_programs_data.py holds it against crp_spmm_plan_host --------

Traits = namedtuple("Traits", "nrow nnz auto_variant team2_min_n team2_pays panels_sparse fill8")


REORDERED = ("band2048",)      # matrices whose programs run under CRPSPMM_REORDER=1: the handle's formats hold the rows in locality order


def traits_of(rp, codes, ncol, reorder=False):
    """What create time decides about a handle (csrc/dispatch.cpp), asked of the library's host-side planner.  reorder: under
    CRPSPMM_REORDER=1, as the handle of a REORDERED matrix is created -- the traits and the panel fill are then those of the rows in
    locality order (the knobs are read live: tests/conftest.py)."""
    import os
    from crp_spmm_amd import hip
    before = os.environ.get("CRPSPMM_REORDER")
    try:
        if reorder:
            os.environ["CRPSPMM_REORDER"] = "1"
        info, _ = hip.spmm_plan_host(rp, codes, [24], ncol=ncol)
        assert bool(info["reordered"]) == bool(reorder), ("the rows' processing order", info)
        f_rp, f_ci = rp, codes
        if reorder:
            perm = hip.locality_order_host(rp, codes, ncol=ncol)[0].astype(np.int64)
            lens = np.diff(rp)[perm]
            f_rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            f_ci = np.concatenate([codes[rp[r]:rp[r + 1]] for r in perm]).astype(np.int32)
        ent = hip.panel_format_host(f_rp, f_ci, np.zeros(codes.size), 8)["real_entries"]
    finally:
        if reorder:
            if before is None:
                del os.environ["CRPSPMM_REORDER"]
            else:
                os.environ["CRPSPMM_REORDER"] = before
    nnz = int(rp[-1])
    return Traits(rp.size - 1, nnz, info["auto_variant"], info["team2_min_n"], bool(info["team2_pays"]), bool(info["panels_sparse"]),
                  nnz / (8.0 * max(ent, 1)))


def resolve_f64(t, n, ld, variant):
    rows = t.nnz > 0 and t.nrow >= 8
    team2 = n >= 24 and n % 2 == 0 and ld % 2 == 0
    v = t.auto_variant if variant == 0 else variant
    wide = n >= t.team2_min_n or (t.team2_min_n == 96 and 61 <= n <= 64)
    if variant == 0 and t.team2_pays and wide and team2:
        v = 5
    panel_or_csr = 3 if (n >= 24 and t.nnz > 0) else 1
    if v == 5:
        return 5 if team2 and rows else panel_or_csr
    G = 4 if n <= 32 else 2
    team2r = 24 <= n <= 128 // G and n % 2 == 0 and ld % 2 == 0
    if variant == 0 and t.team2_pays and t.panels_sparse and n <= 64 and rows and team2r:
        v = 7
    if v == 7:
        return 7 if team2r and rows else panel_or_csr
    if v >= 2 and (n < 24 or t.nnz == 0):
        v = 1
    return v


def resolve_f32(t, n, ld, variant):
    min_n = 65 if t.panels_sparse else 32
    team = (variant == 5 or (variant == 0 and t.team2_pays and n >= min_n)) and t.nnz > 0 and t.nrow >= 8 and \
        n >= 24 and n % 4 == 0 and ld % 4 == 0
    return 5 if team else 1


# ---- the model of one device handle ---------------------------------------------------------------------------------------------

class HandleState:
    """Which lazily built pieces of one crp_csr_dev exist, what built them and in which situation; what a step builds and reads."""

    def __init__(self, traits, transposed):
        self.t, self.transposed = traits, transposed
        self.built = {}                 # piece -> situation it was built in
        self.team_by = None             # "f64" / "f32": fixes team2_compact
        self.situation = "fresh"        # fresh / host / dev: what the last update was (dev: the host copies are stale)
        self.pending = {}               # piece -> kind of the last update since it was last read ... (coverage)
        self.map_state = {}             # piece -> set / changed / cleared since ...
        self.rowmap = 0
        self.last_variant = 0

    # what a product of this shape launches and touches: (resolved variant, pieces read in order of building)
    def product_pieces(self, dtype, variant, n, pad, layout):
        if layout == "cm":
            return None, ()
        ld = n + pad
        if dtype == "f64":
            v = resolve_f64(self.t, n, ld, variant)
            return v, {1: (), 2: ("pan4",), 3: ("pan8",), 5: ("team2",), 7: ("t2r4",) if n <= 32 else ("t2r2",)}[v]
        v = resolve_f32(self.t, n, ld, variant)
        return v, ("val32",) if v == 1 else ("val32", "team2", "tval32")

    def would_build(self, pieces):
        return [p for p in pieces if p not in self.built]

    def touch(self, pieces, dtype, log):
        """a call that needs these pieces: builds the missing ones, reads all of them"""
        for p in pieces:
            if p not in self.built:
                self.built[p] = self.situation
                if p == "team2":
                    self.team_by = dtype
                log.append(("built", self.transposed, p, self.situation, self.team_by if p == "team2" else None))
            else:
                if p in self.pending:
                    log.append(("read_after", self.transposed, p, self.pending.pop(p)))
                if p in self.map_state:
                    log.append(("read_map", self.transposed, p, self.map_state.pop(p)))

    def update(self, src):
        self.situation = src
        for p in self.built:
            self.pending[p] = src

    def set_rowmap(self, which):
        state = "cleared" if which == 0 else ("set" if self.rowmap == 0 else "changed")
        if which != 0 or self.rowmap != 0:
            for p in self.built:
                self.map_state[p] = state
        self.rowmap = which

    @property
    def team2_compact(self):
        """crp_csr_dev_team2_compact: -1 before the team format exists"""
        if "team2" not in self.built:
            return -1
        return int(self.t.fill8 < 0.4 or self.team_by == "f64")


HANDLE_KINDS = ("spmm64", "spmm32", "spmmT64", "spmmT32", "update", "rowmap", "sddmm", "attn", "bwd_q", "bwd_kv", "softmax",
                "softmax_bwd")


def kind_of(step):
    if step[0] == "spmm":
        return "spmm" + ("T" if step[3] == "T" else "") + step[2][1:]
    return step[0]


class HandleModel:
    """Steps of a handle program (stream s in 0, 1, 2; dtype "f64" / "f32"):

        ("spmm", s, dtype, "A" | "T", variant, n, "rm" | "cm", pad)     hip.spmm_csr / spmm_csr_f32 on the handle of A or of A^T
        ("update", s, srcA, srcT, set)                                  update_values on both handles, each from "host" or "dev"
        ("rowmap", s, which)                                            set_rowmap on A's handle: 0 None, 1 / 2 the two maps
        ("sddmm", s, dtype, mode, n, out_pos)                           A.sddmm
        ("attn", s, dtype, bias, widths, out_pos)                       A.attention with lse and p_out; widths indexes ATTN_WIDTHS
        ("bwd_q", s, dtype, bias, widths, out_pos)                      A.attention_bwd_q with ds_out
        ("bwd_kv", s, dtype, bias, widths)                              At.attention_bwd_kv
        ("softmax", s, dtype), ("softmax_bwd", s, dtype)                A.row_softmax / row_softmax_bwd
    """

    def __init__(self, pat, data):
        self.pat, self.data = pat, data
        re = pat.name in REORDERED
        self.A = HandleState(traits_of(pat.rp, pat.codes, pat.ncol0, re), False)
        self.T = HandleState(traits_of(pat.rpt, pat.cit, pat.m, re), True)
        self.cur = 0                    # index of the current value set: the current value vector is data.sets[cur].val
        self.log = []

    @property
    def values(self):
        return self.data.sets[self.cur]

    def rowmap(self):
        """(map or None, c_nrow) of A's handle"""
        if self.A.rowmap == 0:
            return None, self.pat.m
        return self.data.rowmaps[self.A.rowmap]

    def pieces_of(self, step):
        """(handle state, pieces the step needs, dtype) -- what it may build"""
        k = step[0]
        if k == "spmm":
            h = self.T if step[3] == "T" else self.A
            return h, h.product_pieces(step[2], step[4], step[5], step[7], step[6])[1], step[2]
        if k == "sddmm":
            return self.A, ("val32",) if (step[2] == "f32" and step[3] == 1) else (), step[2]
        if k in ("attn", "bwd_q"):
            return self.A, ("val32",) if (step[2] == "f32" and step[3]) else (), step[2]
        if k == "bwd_kv":
            return self.T, ("val32",) if (step[2] == "f32" and step[3]) else (), step[2]
        return self.A, (), None

    def apply(self, step):
        k = step[0]
        if k == "update":
            self.A.update(step[2])
            self.T.update(step[3])
            self.cur = step[4]
        elif k == "rowmap":
            self.A.set_rowmap(step[2])
        else:
            h, pieces, dtype = self.pieces_of(step)
            if k == "spmm":
                v = h.product_pieces(step[2], step[4], step[5], step[7], step[6])[0]
                if v is not None:
                    h.last_variant = v
            h.touch(pieces, dtype, self.log)

    def queries(self):
        """what the queries of the two handles must answer now"""
        return {"A.is_transposed": False, "T.is_transposed": True, "A.team2_compact": self.A.team2_compact,
                "T.team2_compact": self.T.team2_compact}


# ---- the generator of handle programs -------------------------------------------------------------------------------------------

Program = namedtuple("Program", "index seed matrix two_source panel_order set_kinds steps")

HANDLE_PROGRAMS = 8
HANDLE_STEPS = 48
HANDLE_SEED = 20261019
# (matrix, two-source, CRPSPMM_PANEL_ORDER or None) of the eight programs: half of them two-source; two under breadth-first panel
# groups (order 1) on the matrix whose blocks make that order differ from the identity (tests/test_call_programs_data.py shows it)
HANDLE_SETUPS = (("band", False, None), ("band", True, "0"), ("rect", False, None), ("rect", True, None),
                 ("sparse", False, "1"), ("sparse", True, "1"), ("band", True, None), ("sparse", False, None))
# ... and a ninth program, beside the eight: one single-source square matrix of 2048 rows under CRPSPMM_REORDER=1, for the handle's own
# processing order of the rows (crp_csr_dev::ord: f_val, rowmap_fmt, the slot maps re-indexed by the caller's nonzeros)
REORDERED_SETUP = ("band2048", False, None)
SET_KINDS = ("E32", "E64", "E32", "R", "E32", "E64")


def _schedule(index):
    """{(handle, piece): window 0 / 1 / 2} and the update sources of the windows: every handle passes through the three
    situations, the pieces are spread over them by the program's index, and a piece that another one is built on comes no later."""
    first = ("host", "dev") if index % 2 == 0 else ("dev", "host")
    src = {"A": ("fresh", first[0], first[1]), "T": ("fresh", first[1], first[0])}
    team_by = {"A": "f64" if index % 2 == 0 else "f32", "T": "f32" if index % 2 == 0 else "f64"}
    win = {}
    for hi, h in enumerate("AT"):
        for j, p in enumerate(PIECES):
            win[h, p] = (j + index + 2 * hi) % 3
        if team_by[h] == "f32":
            win[h, "tval32"] = win[h, "team2"]
        win[h, "tval32"] = max(win[h, "tval32"], win[h, "team2"])
        win[h, "val32"] = min(win[h, "val32"], win[h, "tval32"])
    return src, team_by, win


def _recipe(rng, h, piece, team_by):
    """a product step (without its stream) that builds the piece on the handle, where it applies to every matrix of this module"""
    pad2 = int(rng.choice((0, 2, 6)))
    if piece == "pan4":
        return ("f64", h, 2, int(rng.choice((24, 26, 32, 40, 64, 130))), "rm", int(rng.choice(PADS)))
    if piece == "pan8":
        return ("f64", h, 3, int(rng.choice((24, 26, 32, 40, 64, 130))), "rm", int(rng.choice(PADS)))
    if piece == "team2":
        if team_by == "f64":
            return ("f64", h, 5, int(rng.choice((24, 26, 32, 40, 64, 130))), "rm", pad2)
        return ("f32", h, 5, int(rng.choice((24, 32, 40, 64))), "rm", 0)
    if piece == "tval32":
        return ("f32", h, 5, int(rng.choice((24, 32, 40, 64))), "rm", 0)
    if piece == "t2r4":
        return ("f64", h, 7, int(rng.choice((24, 26, 32))), "rm", pad2)
    if piece == "t2r2":
        return ("f64", h, 7, int(rng.choice((40, 64))), "rm", pad2)
    return ("f32", h, 1, int(rng.choice(WIDTHS)), "rm", int(rng.choice(PADS)))


def _draw(rng, kind, model):
    """a random step of this kind, without its stream"""
    dt = lambda: str(rng.choice(("f64", "f32")))
    if kind in ("spmm64", "spmmT64"):
        h = "T" if "T" in kind else "A"
        if rng.random() < 0.15:
            return ("spmm", "f64", h, 0, int(rng.choice(WIDTHS)), "cm", int(rng.choice(PADS)))
        return ("spmm", "f64", h, int(rng.choice(VARIANTS64)), int(rng.choice(WIDTHS)), "rm", int(rng.choice(PADS)))
    if kind in ("spmm32", "spmmT32"):
        h = "T" if "T" in kind else "A"
        return ("spmm", "f32", h, int(rng.choice(VARIANTS32)), int(rng.choice(WIDTHS)), "rm", int(rng.choice((0, 0, 1, 2, 4))))
    if kind == "update":
        others = [i for i in range(len(model.data.sets)) if i != model.cur]
        return ("update", str(rng.choice(("host", "dev"))), str(rng.choice(("host", "dev"))), int(rng.choice(others)))
    if kind == "rowmap":
        return ("rowmap", int(rng.choice([w for w in (0, 1, 2) if w != model.A.rowmap])))
    if kind == "sddmm":
        return ("sddmm", dt(), int(rng.integers(0, 2)), int(rng.choice(SD_WIDTHS)), bool(rng.integers(0, 2)))
    if kind in ("attn", "bwd_q"):
        return (kind, dt(), bool(rng.integers(0, 2)), int(rng.integers(0, len(ATTN_WIDTHS))), bool(rng.integers(0, 2)))
    if kind == "bwd_kv":
        return (kind, dt(), bool(rng.integers(0, 2)), int(rng.integers(0, len(ATTN_WIDTHS))))
    return (kind, dt())


def _most_open(kinds, pairs):
    """the kinds after which most ordered pairs are still unseen"""
    left = {k: sum((k, x) not in pairs for x in kinds) for k in kinds}
    return [k for k in kinds if left[k] == max(left.values())]


def _with_stream(step, s):
    return (step[0], s) + tuple(step[1:])


def _handle_program(index, pairs):
    matrix, two_source, order = (HANDLE_SETUPS + (REORDERED_SETUP,))[index]
    seed = HANDLE_SEED + index
    rng = np.random.default_rng(seed)
    pat = pattern(matrix, two_source)
    data = Data(pat, seed, SET_KINDS)
    model = HandleModel(pat, data)
    src, team_by, win = _schedule(index)
    steps = []

    def allowed(step, window):
        """a step may build a piece only in the window the schedule gives it (None: anything goes)"""
        if window is None or step[0] in ("update", "rowmap"):
            return True
        h, pieces, dtype = model.pieces_of(step)
        name = "T" if h.transposed else "A"
        for p in h.would_build(pieces):
            if win[name, p] != window or (p == "team2" and dtype != team_by[name]):
                return False
        return True

    def emit(step):
        step = _with_stream(step, int(rng.integers(0, 3)))
        if steps:
            pairs.add((kind_of(steps[-1]), kind_of(step)))
        model.apply(step)
        steps.append(step)

    def filler(window):
        """a step that builds nothing out of turn, of a kind that closes an ordered pair not seen yet where there is one"""
        prev = kind_of(steps[-1]) if steps else None
        kinds = [k for k in HANDLE_KINDS if k not in ("update", "rowmap") or window is None]
        fresh = [k for k in kinds if (prev, k) not in pairs] or _most_open(kinds, pairs)
        for _ in range(200):
            pool = fresh if _ < 100 else kinds
            step = _draw(rng, str(rng.choice(pool)), model)
            if allowed(_with_stream(step, 0), window):
                return emit(step)
        raise AssertionError("no admissible step")

    for window in range(3):
        if window > 0:
            emit(("update", src["A"][window], src["T"][window], window))           # sets 1 (E64) and 2 (E32)
        todo = [(h, p) for h in "AT" for p in PIECES if win[h, p] == window]
        todo.sort(key=lambda hp: (PIECES.index(hp[1]) not in (2,), rng.random()))   # the team format before what is built on it
        for h, p in todo:
            st = model.T if h == "T" else model.A
            if p in st.built:
                continue
            step = ("spmm",) + _recipe(rng, h, p, team_by[h])
            assert allowed(_with_stream(step, 0), window), (index, window, h, p, step)
            emit(step)
            if rng.random() < 0.5:
                filler(window)
    # the row maps while every piece exists: set, changed, cleared, each followed by products on A that read two of the pieces
    # (which two rotates with the program, so that the eight programs read every piece in every state)
    for si, which in enumerate((1, 2, 0)):
        emit(("rowmap", which))
        for j in range(2):
            p = PIECES[(2 * index + 3 * si + j) % len(PIECES)]
            emit(("spmm",) + _recipe(rng, "A", p, "f64" if p != "team2" else str(rng.choice(("f64", "f32")))))
    while len(steps) < HANDLE_STEPS:
        waiting = [(h, p) for h, st in (("A", model.A), ("T", model.T)) for p in st.pending]
        if waiting and rng.random() < 0.2:              # a piece that has not been read since the last update
            h, p = waiting[int(rng.integers(0, len(waiting)))]
            emit(("spmm",) + _recipe(rng, h, p, (model.T if h == "T" else model.A).team_by))
        else:
            filler(None)
    return Program(index, seed, matrix, two_source, order, SET_KINDS, tuple(steps[:HANDLE_STEPS]))


@functools.lru_cache(maxsize=None)
def handle_programs():
    pairs = set()
    return tuple(_handle_program(i, pairs) for i in range(HANDLE_PROGRAMS))


@functools.lru_cache(maxsize=None)
def reordered_program():
    """the ninth handle program (REORDERED_SETUP); its ordered pairs are its own"""
    return _handle_program(HANDLE_PROGRAMS, set())


def handle_setup(prog):
    """(pattern, data, a fresh model) of a handle program"""
    pat = pattern(prog.matrix, prog.two_source)
    data = Data(pat, prog.seed, prog.set_kinds)
    return pat, data, HandleModel(pat, data)


def literal(prog, upto):
    """the program's prefix up to and including step `upto`, as text a developer can paste into a one-off run"""
    head = "matrix=%r, two_source=%r, panel_order=%r, seed=%d" % (prog.matrix, prog.two_source, prog.panel_order, prog.seed)
    return "# %s\nsteps = [\n%s\n]" % (head, "\n".join("    %r," % (s,) for s in prog.steps[:upto + 1]))


# ---- the engines ----------------------------------------------------------------------------------------------------------------

ENGINE_KINDS = ("exec", "exec_t", "sddmm", "attn", "attn_bwd", "softmax", "softmax_bwd", "update", "update_dev", "set_variant",
                "set_variant_f32", "set_timing")
PARA2D_KINDS = ("exec", "exec_t", "sddmm", "softmax", "update", "update_dev")
# (the backward builds the transposed matrices and its dtype's forward buffer when they are missing: the three sit three apart,
#  so that the generator's schedule gives them one situation)
ENGINE_PIECES = ("exec_t", "sddmm", "softmax", "attn64", "attn32", "exec32", "attn_bwd", "update_dev")
ENGINE_PROGRAMS = {"rp": 6, "para2d": 4}      # (twelve step kinds make 144 ordered pairs: four programs of 40 steps cannot hold them)
ENGINE_STEPS = 40
ENGINE_SEED = 20261119
ENGINE_SETUPS = (("band", 24), ("rect", 40), ("sparse", 26), ("band", 64), ("sparse", 32), ("rect", 7))       # (matrix, glb_n)


class EngineModel:
    """Steps of an engine program (the engine's width glb_n is fixed; ``where`` says where the operands live):

        ("exec", s, dtype, "dev" | "host", layout)          ("exec_t", s, dtype, "dev" | "host", layout)
        ("sddmm", s, dtype, mode, "dev" | "host")           ("attn", s, dtype, bias)            ("attn_bwd", s, dtype, bias)
        ("softmax", s, dtype)   ("softmax_bwd", s, dtype)   ("update", s, set)                  ("update_dev", s, set, dtype)
        ("set_variant", s, v)   ("set_variant_f32", s, v)   ("set_timing", s, on)

    ("sddmm": X, Y and out all on the device or all on the host.)  The 2D engine takes the subset PARA2D_KINDS."""

    def __init__(self, pat, data, n):
        self.pat, self.data, self.n = pat, data, n
        self.cur, self.f32_values = 0, False        # a device update from fp32 leaves the fp32 rounding of the set
        self.built = {}                             # piece -> situation
        self.situation = "fresh"
        self.pending = {}
        self.stale = False
        self.log = []

    def current_values(self):
        v = self.data.sets[self.cur].val
        return v.astype(np.float32).astype(np.float64) if self.f32_values else v

    def kind(self):
        """the kind of the current values: an fp32 device update leaves an E32 set as it is and rounds every other one"""
        k = self.data.sets[self.cur].kind
        return k if (not self.f32_values or k == "E32") else "R"

    def pieces_of(self, step):
        k = step[0]
        if k == "exec":
            return ("exec32",) if step[2] == "f32" else ()
        if k == "exec_t":
            return ("exec_t",)
        if k == "sddmm":
            return ("sddmm",)
        if k == "attn":
            return ("attn64" if step[2] == "f64" else "attn32",)
        if k == "attn_bwd":
            return ("exec_t", "attn64" if step[2] == "f64" else "attn32", "attn_bwd")
        if k in ("softmax", "softmax_bwd"):
            return ("softmax",)
        if k == "update_dev":
            return ("update_dev",)
        return ()

    def apply(self, step):
        k = step[0]
        for p in self.pieces_of(step):
            if p not in self.built:
                self.built[p] = self.situation
                self.log.append(("built", p, self.situation))
                if p == "exec_t":
                    self.stale = False              # the transposed matrices are built from refreshed host values
            elif p in self.pending:
                self.log.append(("read_after", p, self.pending.pop(p)))
        if k == "update":
            self.cur, self.f32_values, self.stale, self.situation = step[2], False, False, "host"
        elif k == "update_dev":
            self.cur, self.f32_values, self.stale, self.situation = step[2], step[3] == "f32", True, "dev"
        if k in ("update", "update_dev"):
            for p in self.built:
                self.pending[p] = self.situation

    def queries(self):
        b = self.built
        return {"transposed_built": "exec_t" in b, "sddmm_built": "sddmm" in b, "attention_built": "attn64" in b or "attn32" in b,
                "attention_bwd_built": "attn_bwd" in b, "row_softmax_built": "softmax" in b, "host_values_stale": self.stale}


def _draw_engine(rng, kind, model):
    dt = lambda: str(rng.choice(("f64", "f32")))
    where = lambda: str(rng.choice(("dev", "dev", "host")))
    if kind in ("exec", "exec_t"):
        return (kind, dt(), where(), int(rng.integers(0, 2)))
    if kind == "sddmm":
        return (kind, dt(), int(rng.integers(0, 2)), where())
    if kind in ("attn", "attn_bwd"):
        return (kind, dt(), bool(rng.integers(0, 2)))
    if kind in ("softmax", "softmax_bwd"):
        return (kind, dt())
    others = [i for i in range(len(model.data.sets)) if i != model.cur]
    if kind == "update":
        return (kind, int(rng.choice(others)))
    if kind == "update_dev":            # from fp32 only an E32 set: any other would leave rounded values, and fewer bitwise checks
        i = int(rng.choice(others))
        return (kind, i, dt() if model.data.sets[i].kind == "E32" else "f64")
    if kind == "set_variant":
        return (kind, int(rng.choice(VARIANTS64)))
    if kind == "set_variant_f32":
        return (kind, int(rng.choice(VARIANTS32)))
    return (kind, bool(rng.integers(0, 2)))


_ENGINE_BUILDERS = {"exec_t": "exec_t", "sddmm": "sddmm", "attn64": "attn", "attn32": "attn", "attn_bwd": "attn_bwd",
                    "softmax": "softmax", "exec32": "exec", "update_dev": "update_dev"}


def _engine_program(index, kinds, pairs, seed0):
    matrix, n = ENGINE_SETUPS[index]
    seed = seed0 + index
    rng = np.random.default_rng(seed)
    pat = pattern(matrix, False)
    data = Data(pat, seed, SET_KINDS)
    model = EngineModel(pat, data, n)
    pieces = [p for p in ENGINE_PIECES if _ENGINE_BUILDERS[p] in kinds]
    order = ("host", "dev") if index % 2 == 0 else ("dev", "host")
    window_of = {"fresh": 0, order[0]: 1, order[1]: 2}
    win = {p: window_of[SITUATIONS[(j + index) % 3]] for j, p in enumerate(pieces)}
    if "update_dev" in win:         # the first device update IS the device situation's opening step
        win["update_dev"] = window_of["dev"]
    steps = []

    def allowed(step, window):
        if window is None:
            return True
        if step[0] in ("update", "update_dev"):
            return False
        return all(win[p] == window for p in model.pieces_of(step) if p not in model.built)

    def emit(step):
        step = _with_stream(step, int(rng.integers(0, 3)))
        if steps:
            pairs.add((steps[-1][0], step[0]))
        model.apply(step)
        steps.append(step)

    def filler(window):
        prev = steps[-1][0] if steps else None
        fresh = [k for k in kinds if (prev, k) not in pairs] or _most_open(kinds, pairs)
        for _ in range(200):
            pool = fresh if _ < 100 else kinds
            step = _draw_engine(rng, str(rng.choice(pool)), model)
            if allowed(_with_stream(step, 0), window):
                return emit(step)
        raise AssertionError("no admissible step")

    def builder(p):
        kind = _ENGINE_BUILDERS[p]
        for _ in range(200):
            step = _draw_engine(rng, kind, model)
            want = {"attn64": "f64", "attn32": "f32", "exec32": "f32"}.get(p)
            if want is None or step[1] == want:
                return step
        raise AssertionError(p)

    for window in range(3):
        if window > 0:
            if order[window - 1] == "host":
                emit(("update", window))
            else:
                emit(("update_dev", window, "f32" if data.sets[window].kind == "E32" else "f64"))
        for p in [p for p in pieces if win[p] == window and p != "update_dev"]:
            if p in model.built:
                continue
            for _ in range(50):                                 # (the backward: of the dtype whose forward buffer is due or there)
                step = builder(p)
                if allowed(_with_stream(step, 0), window):
                    emit(step)
                    break
            if rng.random() < 0.5:
                filler(window)
    while len(steps) < ENGINE_STEPS:
        waiting = [p for p in model.pending if p != "update_dev"]
        if waiting and rng.random() < 0.25:              # a piece that has not been read since the last update
            emit(builder(str(rng.choice(waiting))))
        else:
            filler(None)
    return Program(index, seed, matrix, False, None, SET_KINDS, tuple(steps[:ENGINE_STEPS])), n


@functools.lru_cache(maxsize=None)
def engine_programs(which):
    """the programs of "rp" (RpSpmm) or "para2d" (Para2dSpmm): [(Program, glb_n)]"""
    pairs = set()
    kinds, seed0 = (ENGINE_KINDS, ENGINE_SEED) if which == "rp" else (PARA2D_KINDS, ENGINE_SEED + 100)
    return tuple(_engine_program(i, kinds, pairs, seed0) for i in range(ENGINE_PROGRAMS[which]))


def engine_setup(prog, n):
    pat = pattern(prog.matrix, False)
    data = Data(pat, prog.seed, prog.set_kinds)
    return pat, data, EngineModel(pat, data, n)
