"""CPU: the programs, the value sets and the model of tests/call_programs.py -- what tests/test_gpu_call_programs.py relies on.
Nothing here runs a kernel; the checks concern the programs and the model only."""
import itertools

import numpy as np
import pytest

import call_programs as CP
import fp64_ref


def _all_handle():
    return [(p,) + CP.handle_setup(p) for p in CP.handle_programs()]


def _all_engine(which):
    return [(p, n) + CP.engine_setup(p, n) for p, n in CP.engine_programs(which)]


def _walk_handle():
    """every program's model after its last step"""
    out = []
    for prog, pat, data, model in _all_handle():
        for step in prog.steps:
            model.apply(step)
        out.append((prog, model))
    return out


# ---- the shapes the issue asks for ------------------------------------------------------------------------------------------------

def test_matrices_and_setups(crp, monkeypatch):
    from crp_spmm_amd import hip
    for name in CP.MATRICES:
        for two in (False, True):
            pat = CP.pattern(name, two)
            assert pat.m >= 64 and 200 <= pat.m <= 500, name
            assert np.diff(pat.rp).max() <= 16 and np.diff(pat.rpt).max() <= 16, name
            if two:
                assert (pat.codes < 0).any() and (pat.codes >= 0).any()
                assert (np.diff(pat.gcol)[np.diff(pat.rows) == 0] < 0).any(), "a two-source row keeps ascending columns"
    assert (np.diff(CP.pattern("rect", False).rp) == 0).any()
    # the banded matrix: filled panels, the team formats pay; the third one: mostly holes, variant 0 takes the row-owner kernel
    band, sparse = (CP.traits_of(p.rp, p.codes, p.ncol0) for p in (CP.pattern("band", False), CP.pattern("sparse", False)))
    assert band.team2_pays and not band.panels_sparse and band.auto_variant in (2, 3) and band.fill8 > 0.6
    assert sparse.team2_pays and sparse.panels_sparse and sparse.fill8 < 0.2
    assert [CP.resolve_f64(sparse, n, n, 0) for n in (24, 26, 32, 40, 64)] == [7, 7, 7, 5, 5]       # (from 33 columns: the team kernel)
    setups = CP.HANDLE_SETUPS
    assert len(setups) == CP.HANDLE_PROGRAMS == len(CP.handle_programs()) and sum(s[1] for s in setups) * 2 == len(setups)
    assert {s[0] for s in setups} == set(CP.MATRICES)
    # how the test knows that a CRPSPMM_PANEL_ORDER setting gives a processing order other than the identity: the host view of
    # the very format the handle uploads (crp_panel_format_host runs build_panels with the same knobs) says so
    ordered = [s for s in setups if s[2] == "1"]
    assert len(ordered) >= 2
    for name, two, order in ordered:
        pat = CP.pattern(name, two)
        monkeypatch.setenv("CRPSPMM_PANEL_ORDER", order)
        for R in (4, 8):
            porder = hip.panel_format_host(pat.rp, pat.codes, np.ones(pat.codes.size), R)["porder"]
            assert sorted(porder[porder >= 0]) == list(range(int((porder >= 0).sum()))), "a permutation of the panels"
            assert not np.array_equal(porder, np.arange(porder.size)), (name, two, order, R, "the identity")
        monkeypatch.delenv("CRPSPMM_PANEL_ORDER")
    for prog in CP.handle_programs():
        assert len(prog.steps) <= 48
    for which in ("rp", "para2d"):
        assert len(CP.engine_programs(which)) == CP.ENGINE_PROGRAMS[which] and all(len(p.steps) <= 40 for p, _ in CP.engine_programs(which))


def test_programs_are_reproducible_literals():
    """a program is a pure function of its seed, and its steps print as literals that evaluate back to themselves"""
    CP.handle_programs.cache_clear()
    again = CP.handle_programs()
    for prog in again:
        assert eval(repr(prog.steps)) == prog.steps
        text = CP.literal(prog, 5)
        env = {}
        exec(text, env)
        assert tuple(env["steps"]) == prog.steps[:6]
    first = [p.steps for p in again]
    CP.handle_programs.cache_clear()
    assert [p.steps for p in CP.handle_programs()] == first
    for which in ("rp", "para2d"):
        for prog, _ in CP.engine_programs(which):
            assert eval(repr(prog.steps)) == prog.steps


def test_the_restated_kernel_choice_is_the_library_s(crp):
    """call_programs.resolve_f64 / _f32 against crp_spmm_plan_host on every matrix, width, variant and operand shape it offers"""
    from crp_spmm_amd import hip
    widths = list(CP.WIDTHS) + [48, 96, 128]
    for name, two in itertools.product(CP.MATRICES, (False, True)):
        pat = CP.pattern(name, two)
        for rp, ci, ncol in ((pat.rp, pat.codes, pat.ncol0),) + (((pat.rpt, pat.cit, pat.m),) if not two else ()):
            t = CP.traits_of(rp, ci, ncol)
            for shape, dld in (("aligned", 0), ("ld+1", 1)):
                for v in CP.VARIANTS64:
                    _, got = hip.spmm_plan_host(rp, ci, widths, variant=v, dtype="f64", shape=shape, ncol=ncol)
                    assert got == [CP.resolve_f64(t, n, n + dld, v) for n in widths], (name, two, shape, v)
                for v in CP.VARIANTS32:
                    _, got = hip.spmm_plan_host(rp, ci, widths, variant=v, dtype="f32", shape=shape, ncol=ncol)
                    assert got == [CP.resolve_f32(t, n, n + dld, v) for n in widths], (name, two, shape, v)


# ---- (a) the model's products ----------------------------------------------------------------------------------------------------

def _longdouble_t(pat, val, Bt):
    return fp64_ref.spmm_longdouble(pat.rpt, pat.cit, val[pat.tmap], Bt)


@pytest.mark.parametrize("index", range(CP.HANDLE_PROGRAMS))
def test_model_products_are_the_oracle_s_and_exact(orc, index):
    prog, pat, data, _ = _all_handle()[index]
    rows = pat.rows
    for vs in data.sets:
        if vs.kind == "R":
            continue
        for n in (7, 40, CP.NMAX):
            B, Bt = data.B[:, :n], data.Bt[:, :n]
            want, want_t = data.product(vs, n), data.product_t(vs, n)
            assert np.array_equal(want, orc.spmm_csr(pat.rp, pat.gcol, vs.val, B)), (index, vs.kind, n)
            assert np.array_equal(want_t, orc.spmm_csr(pat.rpt, pat.cit, vs.val[pat.tmap], Bt)), (index, vs.kind, n, "transposed")
            assert np.array_equal(want.astype(np.longdouble), fp64_ref.spmm_longdouble(pat.rp, pat.gcol, vs.val, B)), (index, vs.kind, n)
            assert np.array_equal(want_t.astype(np.longdouble), _longdouble_t(pat, vs.val, Bt)), (index, vs.kind, n, "transposed")
            if vs.kind == "E32":
                for a in (vs.val, B, Bt, want, want_t):
                    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "not exact in fp32"
        for n, mode in itertools.product((7, CP.SD_NMAX), (0, 1)):
            X, Y = data.X[:, :n].astype(np.longdouble), data.Y[:, :n].astype(np.longdouble)
            ref = (X[rows] * Y[pat.gcol]).sum(axis=1) * (vs.val.astype(np.longdouble) if mode else 1)
            want = data.sddmm(vs, mode, n)
            assert np.array_equal(want.astype(np.longdouble), ref), (index, vs.kind, n, mode)
            if vs.kind == "E32":
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want)


# ---- (b) the budgets -------------------------------------------------------------------------------------------------------------

def test_every_exact_budget_holds():
    every = [(p.index, d) for p, _, d, _ in _all_handle()]
    every += [(which, d) for which in ("rp", "para2d") for _, _, _, d, _ in _all_engine(which)]
    tiny = float(np.finfo(np.float32).tiny)
    for tag, data in every:
        assert data.ba >= 10 and data.bb >= 10 and WIDE_FITS(data)
        kinds = [vs.kind for vs in data.sets]
        assert {"E32", "E64", "R"} <= set(kinds) and kinds[0] == "E32"
        for vs in data.sets:
            if vs.kind == "R":
                assert np.abs(vs.val).max() <= 2.0
                continue
            for what, (worst, limit) in data.budgets(vs).items():
                assert worst < limit, (tag, vs.kind, what, worst, limit)
            assert (np.abs(vs.val) >= tiny).all() and np.isfinite(vs.val.astype(np.float32)).all()
            assert (vs.kind == "E32") == np.array_equal(vs.val.astype(np.float32).astype(np.float64), vs.val), \
                "an E64 value must not survive a trip through fp32"


def WIDE_FITS(data):
    return CP.WIDE_BITS + data.bb + int(np.ceil(np.log2(data.longest))) <= 52


# ---- (c) coverage ----------------------------------------------------------------------------------------------------------------

def test_handle_coverage():
    built, read_after, read_map, pairs = set(), set(), set(), set()
    for prog, model in _walk_handle():
        for ev in model.log:
            if ev[0] == "built":
                piece = ev[2] if ev[2] != "team2" else "team2 by " + ev[4]
                built.add((piece, ev[3]))
            elif ev[0] == "read_after":
                read_after.add((ev[2], ev[3]))
            elif ev[0] == "read_map" and not ev[1]:
                read_map.add((ev[2], ev[3]))
        kinds = [CP.kind_of(s) for s in prog.steps]
        pairs |= set(zip(kinds, kinds[1:]))
    pieces = ("pan4", "pan8", "team2 by f64", "team2 by f32", "tval32", "t2r4", "t2r2", "val32")
    missing = [(p, s) for p in pieces for s in CP.SITUATIONS if (p, s) not in built]
    assert not missing, ("never built in this situation", missing)
    missing = [(p, s) for p in CP.PIECES for s in ("host", "dev") if (p, s) not in read_after]
    assert not missing, ("never read after this kind of update", missing)
    missing = [(p, s) for p in CP.PIECES for s in ("set", "changed", "cleared") if (p, s) not in read_map]
    assert not missing, ("never read in this state of the row map", missing)
    missing = [pq for pq in itertools.product(CP.HANDLE_KINDS, repeat=2) if pq not in pairs]
    assert not missing, ("ordered pairs of step kinds that are never adjacent", missing)


@pytest.mark.parametrize("which", ("rp", "para2d"))
def test_engine_coverage(which):
    built, read_after, pairs = set(), set(), set()
    kinds = CP.ENGINE_KINDS if which == "rp" else CP.PARA2D_KINDS
    for prog, n, pat, data, model in _all_engine(which):
        for step in prog.steps:
            assert step[0] in kinds
            model.apply(step)
        for ev in model.log:
            (built if ev[0] == "built" else read_after).add((ev[1], ev[2]))
        pairs |= set(zip([s[0] for s in prog.steps], [s[0] for s in prog.steps[1:]]))
    pieces = [p for p in CP.ENGINE_PIECES if CP._ENGINE_BUILDERS[p] in kinds]
    # (the first device update cannot come after a device update: that piece has two situations)
    missing = [(p, s) for p in pieces for s in CP.SITUATIONS if (p, s) not in built and (p, s) != ("update_dev", "dev")]
    assert not missing, ("never built in this situation", missing)
    missing = [(p, s) for p in pieces for s in ("host", "dev") if (p, s) not in read_after]
    assert not missing, ("never read after this kind of update", missing)
    missing = [pq for pq in itertools.product(kinds, repeat=2) if pq not in pairs]
    assert not missing, ("ordered pairs of step kinds that are never adjacent", missing)


# ---- (d) the share of steps under an exact set ------------------------------------------------------------------------------------

def test_three_quarters_of_the_products_run_under_an_exact_set():
    """Of all product, transposed-product and SDDMM steps at least three quarters run under an E set.  Not every one of those is
    compared bit for bit: an fp32 step under an E64 set rounds the value once and is held to the fp32 bounds (call_programs.exact_in);
    the share that IS compared bitwise is printed beside it."""
    for label, progs in (("handle", [(p, CP.handle_setup(p)[2]) for p in CP.handle_programs()]),
                         ("rp", [(p, CP.engine_setup(p, n)[2]) for p, n in CP.engine_programs("rp")]),
                         ("para2d", [(p, CP.engine_setup(p, n)[2]) for p, n in CP.engine_programs("para2d")])):
        total = exact = bitwise = 0
        for prog, model in progs:
            for step in prog.steps:
                if step[0] in ("spmm", "exec", "exec_t", "sddmm"):
                    total += 1
                    kind = model.kind() if label != "handle" else model.values.kind
                    exact += kind in ("E32", "E64")
                    bitwise += (step[0] == "sddmm" and step[3] == 0) or CP.exact_in(kind, step[2])
                model.apply(step)
        print("%s programs: %d steps, %d under an E set, %d compared bit for bit" % (label, total, exact, bitwise))
        assert total > 0 and 4 * exact >= 3 * total, (label, exact, total)


# ---- the ninth handle program: the rows' processing order -------------------------------------------------------------------------

def test_the_reordered_program_s_handles_hold_their_rows_in_another_order(crp, monkeypatch):
    """how the test knows: under CRPSPMM_REORDER=1 the library's planner reports the locality order as taken for this matrix and its
    transpose (traits_of asserts it), and that order is not the identity"""
    from crp_spmm_amd import hip
    prog = CP.reordered_program()
    assert prog.matrix in CP.REORDERED and not prog.two_source and len(prog.steps) <= 48
    pat, data, model = CP.handle_setup(prog)
    assert pat.m == pat.k >= 2048 and data.longest <= 16
    monkeypatch.setenv("CRPSPMM_REORDER", "1")
    for rp, ci in ((pat.rp, pat.codes), (pat.rpt, pat.cit)):
        perm = hip.locality_order_host(rp, ci, ncol=pat.m)[0]
        assert sorted(perm) == list(range(pat.m)) and not np.array_equal(perm, np.arange(pat.m))
    for vs in data.sets:
        if vs.kind != "R":
            for what, (worst, limit) in data.budgets(vs).items():
                assert worst < limit, (vs.kind, what, worst, limit)
    for step in prog.steps:
        model.apply(step)
    built = {(ev[1], ev[2]) for ev in model.log if ev[0] == "built"}
    assert built == {(t, p) for t in (False, True) for p in CP.PIECES}, "every format on both handles"
    assert {ev[3] for ev in model.log if ev[0] == "read_map" and not ev[1]} == {"set", "changed", "cleared"}
    assert {ev[3] for ev in model.log if ev[0] == "read_after"} == {"host", "dev"}
