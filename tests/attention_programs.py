"""Seeded programs of the multi-head, GAT, GATv2 and dropout calls on one handle pair and on one row engine, with the models that
predict them (no GPU: numpy and the reference modules; helper module of tests/test_attention_programs_data.py,
tests/test_gpu_attention_programs.py and tests/gpu_dist_attention_programs_worker.py; not a conftest).

A second family beside tests/call_programs.py, which it imports from and leaves as it is: the matrices (``pattern``), the value sets
E32 / E64 / R with their exponents and product operands (``Data``), ``seg_sum`` and the ``Program`` tuple are that module's.  What is
new here is the state the newer calls keep between calls:

    handles     the row map of EACH handle inside the dropout key (csrc/dropout.h), and val32 -- the fp32 copy of the values, the bias
                of the fp32 calls -- built lazily on each handle and refreshed by host and device updates
    row engine  the narrow exchange of er (GatXchg, rebuilt when the number of heads changes), the scratch that SDDMM's host ``out``
                shares with every fused call's host ``p_out`` (nnz * heads entries), lse's (rows * heads), the backward's delta
                (rows * heads behind a capacity), B's and C's staging, and the parts' positions, uploaded by whichever of SDDMM, the
                fused attention, GAT, GATv2 or the device update comes first

Operands are drawn as the reference modules draw theirs (attention_ref.operands, gat_ref.operands, gatv2_ref.operands), wide enough
for MAXH heads of the widest head; a call of H heads of dv columns takes the first H * dv columns.

SENSITIVITY, computed here and in the CPU tests from the references alone.  A check can only see a keep bit drawn from the row map
before last if the two maps give different masks, and a bias that went through the wrong value set if the two sets give different
results: ``mask_change`` is the share of keep bits that differ between the handle's current row map and the one before it (the
generator redraws a dropout step below a quarter), ``bias_change`` the share of rows whose reference under the current set leaves
the bound around the reference under the previous one (held to a half by the CPU test for every bias step checked by bounds).
"""
import functools
from collections import Counter

import numpy as np

import attention_ref as R
import call_programs as CP
import dropout_ref as DR
import gat_ref as G
import gatv2_ref as G2

HEADS = (1, 2, 4)
MAXH = 4
GAT_DV = (7, 24, 40)                    # one head's width: both sides of the 16-byte path in both dtypes
DROPS = (0.0, DR.DROP, DR.PIN_DROP)
SEEDS = (DR.SEED, 7)
SLOPE = G.SLOPE
MAX_DK = max(w[0] for w in CP.ATTN_WIDTHS)
MAX_DV = max(max(w[1] for w in CP.ATTN_WIDTHS), max(GAT_DV))
Program = CP.Program
pattern, seg_sum = CP.pattern, CP.seg_sum


class Data:
    """call_programs.Data of the program (value sets, product and SDDMM operands, out_pos, A's row maps) and the operands of the
    newer calls, float64 and read-only; the row maps of the handle of A^T"""

    def __init__(self, pat, seed):
        self.base = base = CP.Data(pat, seed, CP.SET_KINDS)
        self.pat, self.sets, self.out_pos, self.rowmaps = pat, base.sets, base.out_pos, base.rowmaps
        m, k = pat.m, pat.k
        rng = np.random.default_rng(seed + 7700)
        self.rowmapsT = {1: (rng.permutation(k + 29)[:k].astype(np.int32), k + 29), 2: (rng.permutation(k + 3)[:k].astype(np.int32), k + 3)}
        self.Q, self.K, self.V, _ = R.operands(MAXH * MAX_DK, MAXH * MAX_DV, "float64", seed + 1, nrow=m, ncol=k)
        self.dO = rng.standard_normal((m, MAXH * MAX_DV))
        self.el, self.er, self.GV, self.GdO = G.operands("float64", MAXH, MAX_DV, 1.0, seed + 2, nrow=m, ncol=k)
        self.XT, self.XS, self.a, self.XdO = G2.operands("float64", MAXH, MAX_DV, 1.0, seed + 3, nrow=m, ncol=k)
        for x in (self.Q, self.K, self.V, self.dO, self.el, self.er, self.GV, self.GdO, self.XT, self.XS, self.a, self.XdO):
            x.setflags(write=False)

    def rowmap(self, handle, which):
        """(map or None, the rows of the outputs) of a handle in state 0 / 1 / 2"""
        if which == 0:
            return None, (self.pat.m if handle == "A" else self.pat.k)
        return (self.rowmaps if handle == "A" else self.rowmapsT)[which]

    def a_of(self, H, dv):
        """the GATv2 weights of H heads of dv columns: (H, dv), contiguous"""
        return np.ascontiguousarray(self.a.reshape(-1)[:H * dv].reshape(H, dv))


# ---- the masks, by numpy's Philox alone (csrc/dropout.h's key) -------------------------------------------------------------------

def mask_of(data, handle, which, H, drop, seed):
    """(nnz, H) keep bits in the handle's own order of the nonzeros.  A: r = the row after A's map, c = the column code as stored (a
    second-source code as its bit pattern).  A^T: r = the entry's column index (a row of A), c = the handle's row after its map"""
    pat = data.pat
    rm = data.rowmap(handle, which)[0]
    if handle == "A":
        return DR.mask_csr(pat.rp, pat.codes, H, drop, seed, rowmap=rm)
    trow = np.repeat(np.arange(pat.k), np.diff(pat.rpt))
    c = trow if rm is None else rm.astype(np.int64)[trow]
    return DR.keep(seed, pat.cit.astype(np.int64)[:, None], c[:, None], np.arange(H)[None, :], drop)


def mask_change(data, handle, now, before, H, drop, seed):
    """the share of keep bits that differ between the handle's row map now and the one before it"""
    return float((mask_of(data, handle, now, H, drop, seed) != mask_of(data, handle, before, H, drop, seed)).mean())


# ---- the step kinds of a handle program -----------------------------------------------------------------------------------------

ATTN = ("attn", "bwd_q", "bwd_kv")
GATS = ("gat", "gat_row", "gat_col", "gatv2", "gatv2_row", "gatv2_col")
CTRL = ("update", "rowmap", "rowmapT")
PLAIN_KINDS = ATTN + GATS + ("spmm32",)
DROP_KINDS = tuple(k + "/drop" for k in GATS) + ("maskA", "maskT")
HANDLE_KINDS = CTRL + PLAIN_KINDS + DROP_KINDS
ON_T = ("bwd_kv", "gat_col", "gatv2_col")


def kind_of(step):
    """the kind the coverage counts: a GAT / GATv2 step under dropout is a kind of its own, a mask step goes by its handle"""
    k = step[0]
    if k == "mask":
        return "mask" + step[2]
    if k in GATS and step[6] > 0.0:
        return k + "/drop"
    return k


def handle_of(step):
    """"A" or "T": the handle a call step runs on"""
    k = step[0]
    if k in ("mask", "spmm32"):
        return step[2]
    return "T" if k in ON_T else "A"


def dropout_of(step):
    """(H, rate, seed) of a step that draws keep bits, else None"""
    k = step[0]
    if k == "mask":
        return step[3], step[4], step[5]
    if k in GATS and step[6] > 0.0:
        return step[4], step[6], step[7]
    return None


def family_of(kind):
    """"attn", "gat", "gatv2" or "spmm32": the kernels a kind runs"""
    return "gatv2" if kind.startswith("gatv2") else ("gat" if kind.startswith("gat") else ("spmm32" if kind == "spmm32" else "attn"))


def reads_val32(step):
    """whether the step reads the fp32 copy of its handle's values: an fp32 call with the values as bias, a variant-1 fp32 product"""
    k = step[0]
    return k == "spmm32" or (k in ATTN + GATS and step[2] == "f32" and bool(step[3]))


class HandleModel:
    """Steps of a handle program (stream s in 0, 1, 2; dtype "f64" / "f32"; H in HEADS; widths indexes call_programs.ATTN_WIDTHS,
    one head's (dk, dv); dv in GAT_DV, one head's width; drop in DROPS, seed in SEEDS):

        ("update", s, srcA, srcT, set)                          update_values on both handles, each from "host" or "dev"
        ("rowmap", s, which)   ("rowmapT", s, which)            set_rowmap on A's handle / on the handle of A^T: 0 None, 1 / 2 two maps each
        ("attn", s, dtype, bias, H, widths, out_pos)            A.attention(heads=H) with lse and p_out
        ("bwd_q", s, dtype, bias, H, widths, out_pos)           A.attention_bwd_q with ds_out
        ("bwd_kv", s, dtype, bias, H, widths)                   At.attention_bwd_kv
        ("gat", s, dtype, bias, H, dv, drop, seed, out_pos)     A.gat_attention with lse and p_out
        ("gat_row", s, dtype, bias, H, dv, drop, seed, out_pos) A.gat_attention_bwd_row: d_el, delta, ds_out
        ("gat_col", s, dtype, bias, H, dv, drop, seed)          At.gat_attention_bwd_col: d_er, dV
        ("gatv2", ...) ("gatv2_row", ...) ("gatv2_col", ...)    the GATv2 calls: O, lse, p_out / dXT, da_part, delta, ds_out / dXS
        ("mask", s, "A" | "T", H, drop, seed, out_pos)          dropout_mask
        ("spmm32", s, "A" | "T", n)                             a variant-1 fp32 product: the other builder and reader of val32

    A backward step takes O, lse and delta from the forward (and the row side) on a fresh pair at the same arguments, so it runs on
    one handle only.  The model holds the current value set and the one before it, both row maps and the ones before them, and for
    each handle whether val32 exists, in which situation (fresh / host / dev: what the handle's last update was) it was built and
    which kind of update it has not been read after yet."""

    def __init__(self, pat, data):
        self.pat, self.data = pat, data
        self.cur, self.prev = 0, None
        self.map = {"A": 0, "T": 0}
        self.map_before = {"A": None, "T": None}
        self.map_state = {"A": "none", "T": "none"}
        self.val32 = {"A": None, "T": None}
        self.situation = {"A": "fresh", "T": "fresh"}
        self.pending = {"A": {}, "T": {}}          # family of the reader -> the kind of update it has not read val32 after yet
        self.log = []

    @property
    def values(self):
        return self.data.sets[self.cur]

    def apply(self, step):
        k = step[0]
        if k == "update":
            for h, src in (("A", step[2]), ("T", step[3])):
                self.situation[h] = src
                if self.val32[h] is not None:
                    self.pending[h] = {f: src for f in ("attn", "gat", "gatv2", "spmm32")}
            self.prev, self.cur = self.cur, step[4]
            return
        if k in ("rowmap", "rowmapT"):
            h = "A" if k == "rowmap" else "T"
            self.map_state[h] = "cleared" if step[2] == 0 else ("set" if self.map[h] == 0 else "changed")
            self.map_before[h], self.map[h] = self.map[h], step[2]
            return
        h = handle_of(step)
        if reads_val32(step):
            by = "spmm32" if k == "spmm32" else "fused"
            if self.val32[h] is None:
                self.val32[h] = self.situation[h]
                self.log.append(("built", h, self.situation[h], by))
            elif family_of(k) in self.pending[h]:
                self.log.append(("read_after", h, self.pending[h].pop(family_of(k)), k))
        if dropout_of(step) is not None:
            self.log.append(("drop", kind_of(step), h, self.map_state[h]))

    def queries(self):
        return {"A.is_transposed": False, "T.is_transposed": True}


# ---- the generator of handle programs -------------------------------------------------------------------------------------------

HANDLE_PROGRAMS = 8
HANDLE_STEPS = 48
HANDLE_SEED = 20261020
HANDLE_SETUPS = (("band", False), ("band", True), ("rect", False), ("rect", True), ("sparse", False), ("sparse", True), ("band", True),
                 ("sparse", False))
# the window (0 fresh, 1 after the first update, 2 after the second) in which val32 is built on A's handle by program i, and by what;
# the handle of A^T takes the entry of program i + 4.  With the update sources below, each handle's val32 is built in each of
# fresh / host / dev by a fused fp32 bias call and by spmm32 (tests/test_attention_programs_data.py holds it)
VAL32_WINDOW = (0, 0, 1, 1, 1, 1, 2, 2)
VAL32_BUILDER = ("fused", "spmm32", "fused", "fused", "spmm32", "spmm32", "fused", "spmm32")
PAIR_STEPS = 12                         # steps a program may spend on ordered pairs (control, dropout) that no program has yet


def required_pairs():
    """every ordered pair of a control kind and a dropout kind, in both directions"""
    return {(c, d) for c in CTRL for d in DROP_KINDS} | {(d, c) for c in CTRL for d in DROP_KINDS}


def _least(rng, cover, key, options):
    """the option seen least often under this key (ties: at random)"""
    n = [cover[key, o] for o in options]
    pick = [o for o, c in zip(options, n) if c == min(n)]
    return pick[int(rng.integers(0, len(pick)))]


def _draw(rng, kind, model, cover, dtype=None, bias=None):
    """a random step of this kind (of kind_of's names), without its stream; parameters that the coverage counts are the ones seen
    least often so far; dtype, bias: given by the caller (the builders and readers of val32)"""
    base = kind.split("/")[0]
    if kind == "update":
        others = [i for i in range(len(model.data.sets)) if i != model.cur]
        return ("update", str(rng.choice(("host", "dev"))), str(rng.choice(("host", "dev"))), int(rng.choice(others)))
    if kind in ("rowmap", "rowmapT"):
        now = model.map["A" if kind == "rowmap" else "T"]
        return (kind, int(rng.choice([w for w in (0, 1, 2) if w != now])))
    if kind in ("maskA", "maskT"):
        return ("mask", kind[-1], int(_least(rng, cover, ("H", kind), HEADS)), float(_least(rng, cover, ("rate", kind), DROPS[1:])),
                int(_least(rng, cover, ("seed", kind), SEEDS)), bool(rng.integers(0, 2)))
    if kind == "spmm32":
        return ("spmm32", str(_least(rng, cover, ("handle", kind), [h for h in "AT" if model.val32[h] is not None] or ["A"])),
                int(rng.choice((7, 24, 40))))
    dtype = str(_least(rng, cover, ("dtype", kind), ("f64", "f32"))) if dtype is None else dtype
    bias = bool(rng.integers(0, 2)) if bias is None else bias
    H = int(_least(rng, cover, ("H", kind), HEADS))
    if base in ATTN:
        step = (base, dtype, bias, H, int(rng.integers(0, len(CP.ATTN_WIDTHS))))
        return step if base == "bwd_kv" else step + (bool(rng.integers(0, 2)),)
    if kind.endswith("/drop"):
        drop, seed = float(_least(rng, cover, ("rate", kind), DROPS[1:])), int(_least(rng, cover, ("seed", kind), SEEDS))
    else:
        drop, seed = 0.0, int(rng.choice(SEEDS))
    step = (base, dtype, bias, H, int(rng.choice(GAT_DV)), drop, seed)
    return step if base in ON_T else step + (bool(rng.integers(0, 2)),)


def _record(cover, step):
    kind = kind_of(step)
    cover["kind", kind] += 1
    if step[0] in ATTN + GATS:
        cover[("dtype", kind), step[2]] += 1
        cover[("H", kind), step[4]] += 1
    if step[0] == "spmm32":
        cover[("handle", kind), step[2]] += 1
    d = dropout_of(step)
    if d is not None:
        cover[("H", kind), d[0]] += 1
        cover[("rate", kind), d[1]] += 1
        cover[("seed", kind), d[2]] += 1


def _handle_program(index, cover, need):
    matrix, two_source = HANDLE_SETUPS[index]
    seed = HANDLE_SEED + index
    rng = np.random.default_rng(seed)
    pat = pattern(matrix, two_source)
    data = Data(pat, seed)
    model = HandleModel(pat, data)
    first = ("host", "dev") if index % 2 == 0 else ("dev", "host")
    src = {"A": ("fresh", first[0], first[1]), "T": ("fresh", first[1], first[0])}
    win = {"A": VAL32_WINDOW[index], "T": VAL32_WINDOW[(index + 4) % 8]}
    builder = {"A": VAL32_BUILDER[index], "T": VAL32_BUILDER[(index + 4) % 8]}
    steps = []

    def emit(step):
        step = (step[0], int(rng.integers(0, 3))) + tuple(step[1:])
        if steps:
            need.discard((kind_of(steps[-1]), kind_of(step)))
        model.apply(step)
        _record(cover, step)
        steps.append(step)

    def admissible(step, builds):
        """nothing but the scheduled builder builds val32; a dropout step's mask must depend on the handle's last change of row map"""
        full = (step[0], 0) + tuple(step[1:])
        if step[0] in CTRL:
            return True
        h = handle_of(full)
        if reads_val32(full) and model.val32[h] is None and not builds:
            return False
        d = dropout_of(full)
        if d is not None and model.map_before[h] is not None:
            return mask_change(data, h, model.map[h], model.map_before[h], *d) >= 0.25
        return True

    def draw(kind, f32_bias=False, builds=False):
        """an admissible step of this kind; f32_bias: an fp32 call with the values as bias (the builders and readers of val32)"""
        for _ in range(400):
            step = _draw(rng, kind, model, cover, *(("f32", True) if f32_bias else ()))
            if admissible(step, builds):
                return step
        raise AssertionError(("no admissible step", index, kind))

    f32_bias = True
    fused_on = {"A": ("attn", "bwd_q", "gat", "gat_row", "gatv2", "gatv2_row"), "T": ON_T}
    readers = {"A": (("gat", "gat_row"), ("gatv2", "gatv2_row")), "T": (("gat_col",), ("gatv2_col",))}

    def plain_or_drop(base):
        return base if (base in ATTN or rng.random() < 0.5) else base + "/drop"

    for window in range(3):
        if window > 0:
            # (even programs pass through the R set first, odd ones through an E64 set: bias steps are bound-checked under R only)
            emit(("update", src["A"][window], src["T"][window], (3, 1)[(index + window + 1) % 2]))
            for h in "AT":                      # val32 read after this kind of update by a GAT and by a GATv2 bias step
                if model.val32[h] is not None:
                    for family in readers[h]:
                        emit(draw(plain_or_drop(str(rng.choice(family))), f32_bias))
        for h in "AT":
            if win[h] == window:
                if builder[h] == "spmm32":
                    emit(("spmm32", h, int(rng.choice((7, 24, 40)))))
                else:
                    emit(draw(plain_or_drop(fused_on[h][int(rng.integers(0, len(fused_on[h])))]), f32_bias, builds=True))
    # every dropout kind in every state of its handle's row map: this program takes one kind of each handle through set, changed,
    # cleared (the eight programs take all of them)
    on_a = [k for k in DROP_KINDS if k != "maskT" and k.split("/")[0] not in ON_T]
    on_t = [k for k in DROP_KINDS if k == "maskT" or k.split("/")[0] in ON_T]
    ka, kt = on_a[index % len(on_a)], on_t[index % len(on_t)]
    for which in (1, 2, 0):
        emit(("rowmap", which))
        emit(draw(ka))
        emit(("rowmapT", which))
        emit(draw(kt))
    emit(draw("update"))
    for h in "AT":
        for family in readers[h]:
            emit(draw(plain_or_drop(str(rng.choice(family))), f32_bias))
    # ordered pairs (control, dropout) and (dropout, control) that no program has yet
    spent = 0
    while need and spent < PAIR_STEPS and len(steps) < HANDLE_STEPS - 2:
        prev = kind_of(steps[-1])
        nxt = sorted(y for x, y in need if x == prev)
        if nxt:
            emit(draw(nxt[int(rng.integers(0, len(nxt)))]))
            spent += 1
            continue
        x, y = sorted(need)[int(rng.integers(0, len(need)))]
        emit(draw(x))
        spent += 1
    while len(steps) < HANDLE_STEPS:
        emit(draw(str(_least(rng, cover, "kind", PLAIN_KINDS + DROP_KINDS))))
    return Program(index, seed, matrix, two_source, None, CP.SET_KINDS, tuple(steps[:HANDLE_STEPS]))


@functools.lru_cache(maxsize=None)
def handle_programs():
    cover, need = Counter(), required_pairs()
    return tuple(_handle_program(i, cover, need) for i in range(HANDLE_PROGRAMS))


def handle_setup(prog):
    """(pattern, data, a fresh model) of a handle program"""
    pat = pattern(prog.matrix, prog.two_source)
    data = Data(pat, prog.seed)
    return pat, data, HandleModel(pat, data)


def literal(prog, upto):
    """the program's prefix up to and including step `upto`, as text a developer can paste into a one-off run"""
    head = "matrix=%r, two_source=%r, seed=%d" % (prog.matrix, prog.two_source, prog.seed)
    return "# %s\nsteps = [\n%s\n]" % (head, "\n".join("    %r," % (s,) for s in prog.steps[:upto + 1]))


# ---- which checks a handle step gets ------------------------------------------------------------------------------------------------

def bounded(step, model, two_source):
    """whether check c. applies -- the derived bounds of the long-double references: the values do not enter or the set is R, and
    the references can express the call: a step on the handle of A^T under dropout only on a one-source pair without row maps (A's
    forward, whose delta the step reads, then drew the same bits)"""
    k = step[0]
    if k not in ATTN + GATS:
        return False
    if step[3] and model.values.kind != "R":
        return False
    if k in ("gat_col", "gatv2_col") and step[6] > 0.0:
        return not two_source and model.map["A"] == 0 and model.map["T"] == 0
    return True


def forward_reference(data, step, val):
    """the forward's long-double reference of a step's family at the step's arguments under the values `val` (None: no bias):
    (O, its bound), rows by heads * dv -- what bias_change compares"""
    pat = data.pat
    k, dtype, H = step[0], np.dtype({"f64": np.float64, "f32": np.float32}[step[2]]), step[4]
    bias = None if val is None else val.astype(dtype)
    if k in ATTN:
        dk, dv = CP.ATTN_WIDTHS[step[5]]
        O, B = [], []
        for h in range(H):
            ref = R.reference(pat.rp, pat.gcol, data.Q[:, h * dk:(h + 1) * dk].astype(dtype), data.K[:, h * dk:(h + 1) * dk].astype(dtype),
                              data.V[:, h * dv:(h + 1) * dv].astype(dtype), dtype.type(1.0 / np.sqrt(dk)), bias)
            O.append(ref["O"])
            B.append(R.bound_O(ref, dtype))
        return np.concatenate(O, axis=1), np.concatenate(B, axis=1)
    dv = step[5]
    if k.startswith("gatv2"):
        ref = G2.reference(pat.rp, pat.gcol, data.XT[:, :H * dv].astype(dtype), data.XS[:, :H * dv].astype(dtype), data.a_of(H, dv).astype(dtype),
                           SLOPE, bias)
    else:
        ref = G.reference(pat.rp, pat.gcol, data.el[:, :H].astype(dtype), data.er[:, :H].astype(dtype), data.GV[:, :H * dv].astype(dtype), SLOPE, bias)
    return ref["O"]


def bias_change(data, step, cur, prev):
    """the share of rows of A in which the forward's reference under the previous set lies outside the bound around the reference
    under the current set -- the bound the step is held to: a result formed with the previous values would miss it there"""
    a, ba = forward_reference(data, step, data.sets[cur].val)
    b, _ = forward_reference(data, step, data.sets[prev].val)
    return float((np.abs(a - b) > ba).any(axis=1).mean())


# ---- the row engine ------------------------------------------------------------------------------------------------------------------

ENGINE_KINDS = CP.ENGINE_KINDS + ("gat", "gatv2")
ENGINE_PROGRAMS = 4
ENGINE_STEPS = 56
ENGINE_SEED = 20261120
ENGINE_SETUPS = (("band", 24), ("rect", 40), ("sparse", 64), ("band", 26))       # (matrix, glb_n)
ENGINE_LAYOUTS = ("balanced", "balanced", "a rank without rows of A", "a rank without rows of B")     # at several ranks
UPLOADERS = ("sddmm", "gat", "gatv2", "update_dev", "attn", "attn_bwd")       # the calls that upload the parts' positions when they are first
FIRST_UPLOADER = ("sddmm", "gat", "gatv2", "update_dev")                      # of program 0 .. 3


def heads_of(n):
    return tuple(h for h in HEADS if n % h == 0)


class EngineModel(CP.EngineModel):
    """call_programs.EngineModel's steps, the fused attention with heads and operands on either side, and the two newer calls:

        ("attn", s, dtype, bias, H, where)              ("attn_bwd", s, dtype, bias, H)
        ("gat", s, dtype, bias, H, where, layout)       ("gatv2", s, dtype, bias, H, where, layout)

    where: V / XS (for "attn": Q, K and V), O, lse and p_out all on the device ("dev") or all on the host ("host").  The model adds
    the pieces gat64 / gat32 (the narrow exchange of a dtype) and gatv2, the queries gat_built and gatv2_built, the number of heads
    each dtype's exchange was last set up for and which call was the first of UPLOADERS."""

    def __init__(self, pat, data, n):
        super().__init__(pat, data.base, n)
        self.adata = data
        self.gat_heads = {"f64": None, "f32": None}
        self.first_uploader = None

    def pieces_of(self, step):
        k = step[0]
        if k == "gat":
            return ("gat", "gat64" if step[2] == "f64" else "gat32")
        if k == "gatv2":
            return ("gatv2",)
        return super().pieces_of(step)

    def apply(self, step):
        k = step[0]
        if k in UPLOADERS and self.first_uploader is None:
            self.first_uploader = k
        if k == "gat":
            self.gat_heads[step[2]] = step[4]
        if k in ("gat", "gatv2") and step[3]:
            for p in self.pieces_of(step)[:1]:
                if p in self.built and p in self.pending:
                    self.log.append(("bias_after", p, self.pending[p]))
        super().apply(step)

    def queries(self):
        q = super().queries()
        q.update({"gat_built": "gat" in self.built, "gatv2_built": "gatv2" in self.built})
        return q


def _draw_engine(rng, kind, model, several):
    dt = lambda: str(rng.choice(("f64", "f32")))
    where = lambda: str(rng.choice(("dev", "dev", "host")))
    Hs = heads_of(model.n)
    if kind == "attn":
        return (kind, dt(), bool(rng.integers(0, 2)), int(rng.choice(Hs)), where())
    if kind == "attn_bwd":              # at several ranks dK and dV are held to bounds: the values enter under the R set only
        bias = bool(rng.integers(0, 2)) and (not several or model.kind() == "R")
        return (kind, dt(), bias, int(rng.choice(Hs)))
    if kind in ("gat", "gatv2"):
        return (kind, dt(), bool(rng.integers(0, 2)), int(rng.choice(Hs)), where(), int(rng.integers(0, 2)))
    return CP._draw_engine(rng, kind, model)


def _engine_program(index, several):
    matrix, n = ENGINE_SETUPS[index]
    seed = ENGINE_SEED + index + (100 if several else 0)
    rng = np.random.default_rng(seed)
    pat = pattern(matrix, False)
    data = Data(pat, seed)
    model = EngineModel(pat, data, n)
    Hs = heads_of(n)
    d, o = ("f64", "f32") if index % 2 == 0 else ("f32", "f64")
    steps = []

    def emit(step):
        step = (step[0], int(rng.integers(0, 3))) + tuple(step[1:])
        model.apply(step)
        steps.append(step)

    def other_set():
        return int(rng.choice([i for i in range(len(data.sets)) if i != model.cur]))

    def update_dev():
        i = other_set()
        return ("update_dev", i, str(rng.choice(("f64", "f32"))) if data.sets[i].kind == "E32" else "f64")

    rb = lambda: bool(rng.integers(0, 2))
    lay = lambda: int(rng.integers(0, 2))
    where = lambda: str(rng.choice(("dev", "host")))
    gat = lambda dtype, H, bias=None, wh=None: ("gat", dtype, rb() if bias is None else bias, H, where() if wh is None else wh, lay())
    gatv2 = lambda dtype, H, bias=None, wh=None: ("gatv2", dtype, rb() if bias is None else bias, H, where() if wh is None else wh, lay())
    host_sddmm = lambda dtype: ("sddmm", dtype, int(rng.integers(0, 2)), "host")

    # the first uploader of the parts' positions, after calls that upload nothing; then gat_built and gatv2_built first set in the
    # situations the four programs spread over fresh / host / dev
    emit(("exec", d, "dev", 0))
    emit(("softmax", o))
    first = FIRST_UPLOADER[index]
    if first == "sddmm":
        emit(("sddmm", d, 1, "dev"))
        emit(gat(d, Hs[0]))                     # fresh
        emit(("update", other_set()))
        emit(gatv2(o, Hs[-1]))                  # host
    elif first == "gat":
        emit(gat(d, Hs[0]))                     # fresh
        emit(update_dev())
        emit(gatv2(o, Hs[-1]))                  # dev
    elif first == "gatv2":
        emit(gatv2(d, Hs[-1]))                  # fresh
        emit(("update", other_set()))
        emit(gat(o, Hs[0]))                     # host
    else:
        emit(update_dev())
        emit(gat(d, Hs[0]))                     # dev
        emit(gatv2(o, Hs[-1]))                  # dev
    # gat and gatv2 with the values as bias after each kind of update
    for upd in (("update", other_set()), None):
        emit(upd if upd is not None else update_dev())
        emit(gat(str(rng.choice((d, o))), int(rng.choice(Hs)), True))
        emit(gatv2(str(rng.choice((d, o))), int(rng.choice(Hs)), True))
    # the narrow exchange of dtype d across changes of H: an increase, a decrease, returns to earlier values; a gat of the other dtype,
    # an exec, an attn, an sddmm with a host out and a device update between two of them
    a, b, c = (Hs + Hs)[:3] if len(Hs) < 3 else Hs
    seq = (a, b, c, b, a, c, a) if len(Hs) == 3 else (a, b, a, b, a, b, a)
    between = (None, gat(o, seq[-2]), ("exec", o, where(), lay()), ("attn", d, rb(), int(rng.choice(Hs)), where()), host_sddmm(o), update_dev())
    for j, H in enumerate(seq):
        if j > 0 and between[j - 1] is not None:
            emit(between[j - 1])
        emit(gat(d, H))
    if 4 in Hs:
        # p_out staged in the scratch that SDDMM's host out shares: H = 4 before and after a host-out sddmm, and before and after a
        # host p_out of one head of the other dtype; the fused call rotates with the program
        big = {0: lambda dt, H: ("attn", dt, rb(), H, "host"), 1: lambda dt, H: gat(dt, H, None, "host"),
               2: lambda dt, H: gatv2(dt, H, None, "host")}[index % 3]
        emit(big(d, 4))
        emit(host_sddmm(o))
        emit(big(d, 4))
        emit(big(o, 1))
        emit(big(d, 4))
        # the backward's delta behind its capacity: H = 4 before H = 1 and after it, per dtype
        for dtype in (d, o):
            for H in (4, 1, 4):
                emit(("attn_bwd", dtype, rb() and (not several or model.kind() == "R"), H))
    kinds = [k for k in ENGINE_KINDS]
    while len(steps) < ENGINE_STEPS:
        emit(_draw_engine(rng, str(rng.choice(kinds)), model, several))
    return Program(index, seed, matrix, False, None, CP.SET_KINDS, tuple(steps[:ENGINE_STEPS])), n


@functools.lru_cache(maxsize=None)
def engine_programs(several):
    """the programs of the row engine at one rank (several False) or at several ranks (True): [(Program, glb_n)]; program i of the
    several-rank family runs on ENGINE_LAYOUTS[i]"""
    return tuple(_engine_program(i, bool(several)) for i in range(ENGINE_PROGRAMS))


def engine_setup(prog, n):
    pat = pattern(prog.matrix, False)
    data = Data(pat, prog.seed)
    return pat, data, EngineModel(pat, data, n)


def partition(layout, rp, world, k):
    """(row displacements of A, of B) of ENGINE_LAYOUTS' layout on `world` ranks: A's rows by planner.csr_mat_row_partition, B's k rows
    with them where the matrix is square and evenly otherwise; the hole is the one the other engine workers cut (rank 0 without rows
    at two ranks, else rank 1)"""
    from crp_spmm_amd import planner
    m = rp.size - 1
    rb = np.array(planner.csr_mat_row_partition(rp, world))
    bd = rb.copy() if k == m else (np.arange(world + 1) * k) // world

    def hole(d):
        d = d.copy()
        if world > 1:
            d[1] = d[0] if world == 2 else d[2]
        return d
    if layout == "a rank without rows of A":
        rb = hole(rb)
    elif layout == "a rank without rows of B":
        bd = hole(bd)
    return rb, bd
